"""The normal operator G = P^T P as an operator line of the kept-basis solves, and
Handle.svds on top of it.

normal_apply is held per element to the gamma bound of its two sums.  The solves run
beside the NumPy restatement of the restart loop (restated_cycles of test_gpu_restart with
mul = Q -> P^T (P Q)) from the same uniform_B start block, under svds' stop test est_i <=
tol sigma_max max(sigma_i, sqrt(eps) sigma_max): fp64 meets absolute bounds, fp32 and the
orthogonality figures are held to 100 x the restatement's, the project's convention.  The
matrices are built here in NumPy (rect); the dense SVD is NumPy's."""
import numpy as np
import pytest

from test_gpu_restart import f64, host_panel, restated_cycles, wanted

pytestmark = pytest.mark.gpu

EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
NPDT = {"f64": np.float64, "f32": np.float32}
LC = 5

CASES = {  # name: (R, C, b, m, keep, k, dtype, tol, planted entries)
    "tall": (1500, 1024, 16, 6, 2, 24, "f64", 1e-10, 24),
    "wide": (1024, 1500, 16, 6, 2, 24, "f64", 1e-10, 24),  # runs on A A^T
    "b5": (901, 777, 5, 12, 5, 13, "f64", 1e-10, 8),
    "b32f": (1500, 1024, 32, 4, 1, 24, "f32", 2e-5, 24),
}


def rect(lz, R, C, nplant, dt):
    """Every row 8 random entries in sorted distinct columns (none in every 97th row), then
    entry ((7 + 42 i) mod R, (3 + 29 i) mod C) set to 4 + 2 i for i < nplant.  Returns the
    CsrHost and the dense copy (fp64 of the stored values)."""
    rng = np.random.default_rng(5)
    S = np.zeros((R, C))
    for i in range(R):
        if i % 97 == 0:
            continue
        cols = np.sort(rng.choice(C, 8, replace=False))
        S[i, cols] = rng.uniform(-1, 1, 8)
    for i in range(nplant):
        S[(7 + 42 * i) % R, (3 + 29 * i) % C] = 4 + 2 * i
    S = S.astype(NPDT[dt])
    rows, cols = np.nonzero(S)
    rp = np.zeros(R + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=R))
    return lz.CsrHost(R, rp, cols.astype(np.int32), S[rows, cols]), S.astype(np.float64)


class Problem:
    pass


_mats, _cache = {}, {}


def matrix(lz, R, C, nplant, dt):
    key = (R, C, nplant, dt)
    if key not in _mats:
        _mats[key] = rect(lz, R, C, nplant, dt)
    return _mats[key]


def svd_figures(Pd, Q, T, bm, b, k, eps, sdense):
    """What the tests measure from a basis Q of the solve on G = Pd^T Pd, its projected T and
    beta_m (fp64 copies): svds' stop ratio, the singular values, the true residuals ||Pd^T y -
    sigma x|| against their estimate est / sigma, and the orthogonality of both sides."""
    theta, Sv = wanted(T, k, "largest")
    est = np.linalg.norm(bm @ Sv[-b:], axis=0)
    smax = float(np.sqrt(np.abs(np.linalg.eigvalsh(0.5 * (T + T.T))).max()))
    sig = np.sqrt(np.maximum(theta, 0.0))
    ratio = est / (smax * np.maximum(sig, np.sqrt(eps) * smax))
    X = Q @ Sv
    Y = Pd @ X
    Y = Y / np.linalg.norm(Y, axis=0)
    true = np.linalg.norm(Pd.T @ Y - X * sig, axis=0)
    return dict(ratio=float(ratio.max()), smax=smax, sig=sig, true=true,
                gap=float(np.abs(true - est / sig).max()), sig_err=float(np.abs(sig - sdense[:k]).max()),
                xo=float(np.abs(X.T @ X - np.eye(k)).max()), yo=float(np.abs(Y.T @ Y - np.eye(k)).max()),
                orth=float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max()))


def problem(lz, torch, name):
    """The operator, its dense copy and singular values, the start block, and the restatement
    run to svds' stop test (figures after every cycle), once per shape."""
    if name in _cache:
        return _cache[name]
    R, C, b, m, r, k, dt, tol, npl = CASES[name]
    s = Problem()
    s.npdt, s.tdt, s.eps = NPDT[dt], (torch.float64 if dt == "f64" else torch.float32), EPS[dt]
    s.A, s.S = matrix(lz, R, C, npl, dt)
    s.Ad = lz.CsrDevice.from_host(s.A, n_cols=C)
    s.Pd = s.S if C <= R else s.S.T  # the solve runs on G = Pd^T Pd, n = min(R, C)
    s.n, s.p = s.Pd.shape[1], s.Pd.shape[0]
    s.sdense = np.linalg.svd(s.S, compute_uv=False)
    s.Bh = lz.uniform_B(s.n, b, dtype=s.npdt)
    s.vs = -(-s.n * b // 4) * 4
    Pp = s.Pd.astype(s.npdt)
    s.ref = []
    for Q, T, bm in restated_cycles(lambda Q: Pp.T @ (Pp @ Q), s.Bh, b, m, r, "largest", 2, s.npdt):
        s.ref.append(svd_figures(s.Pd, Q, T, bm, b, k, s.eps, s.sdense))
        if s.ref[-1]["ratio"] <= tol:
            break
        assert len(s.ref) < 40, "the restatement does not converge"
    s.cycles_ref = len(s.ref)
    _cache[name] = s
    return s


@pytest.mark.parametrize("b,dt", [(16, "f64"), (32, "f32"), (5, "f64")])
@pytest.mark.parametrize("R,C", [(1500, 1024), (1024, 1500)])
def test_normal_apply(lz, handle, torch_cuda, R, C, b, dt):
    """Y = S^T (S X) per element within 8 (k_A + k_t + 4) eps (|S^T| |S| |X|): k_A the longest
    row of P = S, k_t the length of the output row's row of Pt.  X is unchanged, Y starts as NaN."""
    torch = torch_cuda
    A, S = matrix(lz, R, C, 24, dt)
    P = lz.CsrDevice.from_host(A, n_cols=C)
    Pt = P.transpose(handle)
    rng = np.random.default_rng(11)
    Xh = rng.uniform(-1, 1, (C, b)).astype(NPDT[dt])
    X = torch.from_numpy(Xh).cuda()
    Y = torch.full((C, b), float("nan"), dtype=X.dtype, device="cuda")
    work = torch.full((R * b,), float("nan"), dtype=X.dtype, device="cuda")
    handle.normal_apply(P, Pt, X, Y, work)
    got = f64(Y.cpu().numpy())
    Xd = f64(Xh)
    ref = S.T @ (S @ Xd)
    k_A = int(np.diff(A.row_ptr).max())
    k_t = np.diff(Pt.row_ptr.cpu().numpy())[:, None]
    bound = 8 * (k_A + k_t + 4) * EPS[dt] * (np.abs(S.T) @ (np.abs(S) @ np.abs(Xd)))
    err = np.abs(got - ref)
    print(f"normal_apply {R}x{C} b={b} {dt}: max err {err.max():.3e}, max err/bound "
          f"{(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert torch.equal(X, torch.from_numpy(Xh).cuda())


@pytest.mark.parametrize("name", ["tall", "b5"])
def test_resume_on_G(lz, handle, torch_cuda, name):
    """One cycle, the host restart, the compress, one resumed cycle, all on G = P^T P: the basis
    is orthonormal and Q^T G Q (G dense in NumPy) is the T of restart_coeffs + restart_fill."""
    torch = torch_cuda
    R, C, b, m, r, k, dt, tol, _ = CASES[name]
    s = problem(lz, torch, name)
    n, p, vs = s.n, s.p, s.vs
    kw = dict(dtype=s.tdt, device="cuda")
    At = s.Ad.transpose(handle)
    Pm, Pt = (s.Ad, At) if C <= R else (At, s.Ad)
    normal = (Pm, Pt, torch.full((p * b,), float("nan"), **kw))
    V = torch.full((m * vs,), float("nan"), **kw)
    W = torch.empty(n, b, **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(None, torch.from_numpy(s.Bh).cuda(), m, LC, q, al, be, V, vs, W, passes=2,
                                normal=normal)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.Assemble_T(m, b, alpha, beta)
    _, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], "largest")
    handle.panel_compress(V, vs, m, r, torch.from_numpy(Z).to(**kw), n=n)
    q[:r * b] = torch.from_numpy(f64(q.cpu().numpy()) @ Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)).to(**kw)
    handle.block_lanczos_reorth_resume(None, r, m, LC, torch.from_numpy(sigma).to(**kw), q, al, be, V, vs, W,
                                       passes=2, normal=normal)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.restart_fill(r, m, b, alpha, beta, Tn)
    Q = host_panel(V, m, vs, n, b)
    assert np.isfinite(Q).all()
    G = s.Pd.T @ s.Pd
    norm1 = float(np.abs(G).sum(axis=0).max())
    ref = s.ref[1]
    orth = float(np.abs(Q.T @ Q - np.eye(m * b)).max())
    dT = float(np.abs(Q.T @ G @ Q - T).max())
    print(f"{name}: after one restart on G max|Q^T Q - I| = {orth:.3e} (restatement {ref['orth']:.3e}), "
          f"max|Q^T G Q - T| = {dT:.3e} (bound {1e-10 * norm1:.3e})")
    assert orth <= 100 * ref["orth"]
    assert dT <= 1e-10 * norm1
    qd = f64(q.cpu().numpy())
    assert np.array_equal(qd[r * b:], Q[LC, r * b:]), "q = row lc of every new Q_j"


def run_svds(handle, torch, name, s, **kw):
    R, C, b, m, r, k, dt, tol, _ = CASES[name]
    args = dict(b=b, m=m, keep=r, tol=tol, max_cycles=2 * s.cycles_ref, B=torch.from_numpy(s.Bh).cuda(), lc=LC,
                passes=2)
    args.update(kw)
    return handle.svds(s.Ad, k, **args)


@pytest.mark.parametrize("name", list(CASES))
def test_svds(lz, handle, torch_cuda, name):
    torch = torch_cuda
    R, C, b, m, r, k, dt, tol, _ = CASES[name]
    s = problem(lz, torch, name)
    ref = s.ref[-1]
    out = run_svds(handle, torch, name, s)
    nch = -(-k // b)
    print(f"{name}: device {out['cycles']} cycles, {out['n_spmm']} SpMMs (restatement {s.cycles_ref} cycles); "
          "per-cycle stop ratio " + " ".join(f"{x:.1e}" for x in out["history"]))
    assert out["converged"] and abs(out["cycles"] - s.cycles_ref) <= 1
    assert len(out["history"]) == out["cycles"]
    steps = m + (out["cycles"] - 1) * (m - r)
    assert out["n_spmm"] == 2 * steps + 2 * nch
    # heights: U has R-row blocks, V C-row blocks, in both orientations
    assert out["ustride"] >= R * b and out["U"].numel() == nch * out["ustride"]
    assert out["vstride"] >= C * b and out["V"].numel() == nch * out["vstride"]
    assert (out["At"].n, out["At"].n_cols) == (C, R)
    Up = host_panel(out["U"], nch, out["ustride"], R, b)
    Vp = host_panel(out["V"], nch, out["vstride"], C, b)
    assert np.isfinite(Up).all() and np.isfinite(Vp).all()
    assert (Up[:, k:] == 0).all() and (Vp[:, k:] == 0).all(), "the last block is zero-padded"
    U, V, sig = Up[:, :k], Vp[:, :k], out["s"]
    assert (np.diff(sig) <= 0).all()
    smax = float(s.sdense[0])
    err = np.abs(sig - s.sdense[:k])
    # what svds measures is ||Pt y - sigma x||: ||A^T u - sigma v|| on A^T A, ||A v - sigma u|| on A A^T
    true = np.linalg.norm(s.S.T @ U - V * sig, axis=0) if C <= R else np.linalg.norm(s.S @ V - U * sig, axis=0)
    uo = float(np.abs(U.T @ U - np.eye(k)).max())
    vo = float(np.abs(V.T @ V - np.eye(k)).max())
    # the restatement's x side is V when the solve ran on A^T A, U when on A A^T
    ref_uo, ref_vo = (ref["yo"], ref["xo"]) if C <= R else (ref["xo"], ref["yo"])
    gap = max(ref["gap"], s.eps * smax)
    print(f"{name}: max|sigma - dense| {err.max():.3e} (restatement {ref['sig_err']:.3e}), measured resid "
          f"{out['resid'].max():.3e}, from U, V here {true.max():.3e} (restatement true {ref['true'].max():.3e}, "
          f"gap {ref['gap']:.3e}), max|U^T U - I| {uo:.3e} (restatement {ref_uo:.3e}), max|V^T V - I| {vo:.3e} "
          f"(restatement {ref_vo:.3e})")
    if dt == "f64":
        assert (err <= tol * smax).all()
    else:
        assert err.max() <= 100 * ref["sig_err"]
    assert out["resid"].max() <= tol * smax + 100 * gap
    assert true.max() <= tol * smax + 100 * gap, "the residual measured here from U, V and s"
    assert uo <= 100 * max(ref_uo, s.eps) and vo <= 100 * max(ref_vo, s.eps)
    out2 = run_svds(handle, torch, name, s)
    assert out2["cycles"] == out["cycles"] and np.array_equal(out2["s"], sig)
    assert torch.equal(out2["U"], out["U"]) and torch.equal(out2["V"], out["V"])


def test_max_cycles_returns_unconverged(lz, handle, torch_cuda):
    s = problem(lz, torch_cuda, "tall")
    assert s.cycles_ref > 1
    out = run_svds(handle, torch_cuda, "tall", s, max_cycles=1)
    assert out["converged"] is False and out["cycles"] == 1 and len(out["history"]) == 1


def test_rejected(lz, handle, torch_cuda):
    torch = torch_cuda
    R, C, b, m, r, k, dt, tol, _ = CASES["tall"]
    s = problem(lz, torch, "tall")
    with pytest.raises(lz.LanczosError):
        handle.svds(s.Ad, k, b=b, m=m, keep=1)   # keep * b < k
    with pytest.raises(lz.LanczosError):
        handle.svds(s.Ad, k, b=b, m=2, keep=2)   # keep >= m
    n, p, vs = s.n, s.p, s.vs
    kw = dict(dtype=torch.float64, device="cuda")
    At = s.Ad.transpose(handle)
    V, W, B = torch.zeros(m * vs, **kw), torch.empty(n, b, **kw), torch.from_numpy(s.Bh).cuda()
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    sg = torch.zeros(r, b, b, **kw)
    work = torch.empty(p * b, **kw)
    cheb_work = torch.empty(2 * n * b, **kw)

    def first(normal, **extra):
        handle.block_lanczos_reorth(None, B, m, LC, q, al, be, V, vs, W, normal=normal, **extra)

    def resume(normal, **extra):
        handle.block_lanczos_reorth_resume(None, r, m, LC, sg, q, al, be, V, vs, W, normal=normal, **extra)

    for call in (first, resume):
        with pytest.raises(lz.LanczosError):
            call((s.Ad, At, work), filt=(4, 0.0, 1.0, 2.0), work=cheb_work)  # normal= with filt=
        with pytest.raises(lz.LanczosError):
            call((s.Ad, At, work[:p * b - 1]))                               # work too small
        with pytest.raises(lz.LanczosError):
            call((s.Ad, At, work.to(torch.float32)))                         # work of the wrong dtype
    # the ABI's own checks: work NULL, work overlapping W
    L, ptr = handle.L, lambda t: t.data_ptr()

    def raw(work_ptr):
        return L.lz_block_lanczos_reorth_normal(handle.ptr, n, p, s.Ad.nnz, ptr(s.Ad.row_ptr), ptr(s.Ad.col),
                                                ptr(s.Ad.val), ptr(At.row_ptr), ptr(At.col), ptr(At.val), lz.LZ_F64, b,
                                                m, LC, ptr(B), ptr(q), ptr(al), ptr(be), ptr(V), vs, ptr(W), 2,
                                                work_ptr)

    assert raw(None) == -1 and L.lz_last_error()
    assert raw(ptr(W)) == -1 and L.lz_last_error()
    assert raw(ptr(V) + 16) == -1 and L.lz_last_error()
