"""Thick-restart block Lanczos: the in-place panel compress (lz_panel_compress), the
resumed solve (lz_block_lanczos_reorth_resume) and the driver loop (Handle.eigsh).

Compress: inputs uniform in (-1, 1), reference NumPy fp64 einsum, the tolerances of
test_panel_apply: fp64 8 (k b) eps64 (the gamma bound of a length k b sum of products of
magnitude <= 1), fp32 4 eps32 sum|v||z| per entry (sums are fp64, rounded once).
Solver: a NumPy restatement of the same loop (eigh for the sqrtm and for T) runs beside
the device.  fp64 runs meet the absolute bounds of the issue; orthogonality, and every
figure of the fp32 run, are held to 100 x the restatement's figure at the same point.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)

# (n, b, k, r, dtype, pad): r = k is the in-place hazard case; k = 17, 64 walk many
# input blocks through the two staging buffers; pad = 32: vstride = n*b + 32, NaN padding
COMPRESS_CASES = [
    (1, 16, 1, 1, "f64", 0),
    (15, 16, 3, 2, "f64", 0),
    (17, 16, 2, 1, "f64", 32),
    (4099, 16, 16, 16, "f64", 0),
    (4099, 16, 17, 16, "f64", 32),
    (4099, 16, 64, 16, "f64", 0),
    (4099, 16, 16, 4, "f64", 32),
    (1000, 5, 7, 3, "f64", 32),
    (1000, 32, 3, 2, "f32", 0),
    (1000, 16, 4, 4, "f32", 32),
]
IDS = ["n%d-b%d-k%d-r%d-%s-pad%d" % c for c in COMPRESS_CASES]


def test_constants(lz):
    assert (lz.PANEL_MAX_KEEP, lz.PANEL_MAX_BLOCKS) == (16, 64)
    assert (lz.LZ_K_PCOMP16, lz.LZ_K_PCOMP_GEN) == (11, 12)


@pytest.mark.parametrize("n,b,k,r,dt,pad", COMPRESS_CASES, ids=IDS)
def test_panel_compress(lz, handle, torch_cuda, n, b, k, r, dt, pad):
    torch = torch_cuda
    npdt = np.float64 if dt == "f64" else np.float32
    rng = np.random.default_rng(300 + n + k + r)
    Vh = rng.uniform(-1, 1, (k, n, b)).astype(npdt)
    Zh = rng.uniform(-1, 1, (r, k, b, b)).astype(npdt)
    vs = n * b + pad
    buf = np.full(k * vs, np.nan, npdt)
    for j in range(k):
        buf[j * vs:j * vs + n * b] = Vh[j].ravel()
    Z = torch.from_numpy(Zh).cuda()
    V = torch.from_numpy(buf).cuda()
    handle.panel_compress(V, vs, k, r, Z, n=n)
    assert handle.last_kernel()[1] == (lz.LZ_K_PCOMP16 if (b == 16 and dt == "f64") else lz.LZ_K_PCOMP_GEN)
    out = V.cpu().numpy().reshape(k, vs)
    got = out[:r, :n * b].reshape(r, n, b).astype(np.float64)
    V64, Z64 = Vh.astype(np.float64), Zh.astype(np.float64)
    ref = np.einsum("jri,cjid->crd", V64, Z64)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), "NaN / Inf in the kept blocks"
    if dt == "f64":
        tol = 8 * (k * b) * EPS64
        print(f"panel_compress {n}x{b} k={k} r={r}: max err {err.max():.3e} (tol {tol:.3e})")
        assert err.max() <= tol
    else:
        bound = 4 * EPS32 * np.einsum("jri,cjid->crd", np.abs(V64), np.abs(Z64))
        print(f"panel_compress {n}x{b} k={k} r={r} fp32: max err/bound {(err / bound).max():.3e}")
        assert (err <= bound).all()
    # blocks r .. k-1 bitwise unchanged; the padding still NaN and nothing else
    assert np.array_equal(out[r:, :n * b], buf.reshape(k, vs)[r:, :n * b])
    assert np.isnan(out[:, n * b:]).all() and np.isfinite(out[:, :n * b]).all()
    V2 = torch.from_numpy(buf).cuda()
    handle.panel_compress(V2, vs, k, r, Z, n=n)
    assert torch.equal(V.view(k, vs)[:, :n * b], V2.view(k, vs)[:, :n * b]), "two identical calls must agree bitwise"


def test_compress_past_4gib(lz, handle, torch_cuda):
    """A 4.4 GB panel: every block past the seventh starts beyond a 32-bit byte offset.
    Filled on the device; reference torch fp64 products on the device."""
    torch = torch_cuda
    n, b, k, r = (1 << 20) + 3, 16, 33, 2
    vs = n * b
    assert k * vs * 8 > (1 << 32)
    g = torch.Generator(device="cuda").manual_seed(4343)
    V = torch.rand(k * vs, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    Z = torch.rand(r, k, b, b, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    Vv = V.view(k, n, b)
    ref = torch.zeros(r, n, b, dtype=torch.float64, device="cuda")
    for c in range(r):
        for j in range(k):
            ref[c].addmm_(Vv[j], Z[c, j])
    tail = V[r * vs:].clone()
    handle.panel_compress(V, vs, k, r, Z)
    assert handle.last_kernel()[1] == lz.LZ_K_PCOMP16
    err = float((Vv[:r] - ref).abs().max())
    print(f"4 GiB panel_compress: max err {err:.3e} (tol {8 * k * b * EPS64:.3e})")
    assert err <= 8 * k * b * EPS64
    assert torch.equal(V[r * vs:], tail), "blocks r .. k-1 are not written"


@pytest.mark.parametrize("k,r", [(5, 3), (8, 7), (16, 16), (3, 1)])
def test_compress_many_units(lz, handle, torch_cuda, k, r):
    """More row units than workgroups at each accumulator shape of the MFMA kernel (r <= 4,
    <= 8, <= 16: 512, 256, 128 rows per unit): a workgroup walks several units, with the
    staging of coefficients and tiles carried from one unit into the next.  n is odd, so the
    last unit is partial.  Checked on the device against torch fp64 products."""
    torch = torch_cuda
    n, b = 300007, 16
    vs = n * b + 32
    g = torch.Generator(device="cuda").manual_seed(5000 + 17 * k + r)
    V = torch.rand(k * vs, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    Z = torch.rand(r, k, b, b, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    V0 = V.clone()
    blocks = V0.view(k, vs)[:, :n * b].reshape(k, n, b)
    ref = torch.einsum("jri,cjid->crd", blocks, Z)
    handle.panel_compress(V, vs, k, r, Z, n=n)
    assert handle.last_kernel()[1] == lz.LZ_K_PCOMP16
    got = V.view(k, vs)[:r, :n * b].reshape(r, n, b)
    err = float((got - ref).abs().max())
    print(f"panel_compress {n}x{b} k={k} r={r}: max err {err:.3e} (tol {8 * k * b * EPS64:.3e})")
    assert err <= 8 * k * b * EPS64
    assert torch.equal(V.view(k, vs)[r:], V0.view(k, vs)[r:]) and torch.equal(V.view(k, vs)[:, n * b:], V0.view(k, vs)[:, n * b:])


# ------------------------------------------------------------------ solver
def planted(lz, n, nplant, npdt):
    """gen_banded(n, 9 nnz/row, halfwidth 32) with 4 + 2i added to the diagonal of row 7 + 42i."""
    A = lz.gen_banded(n, nnz_per_row=9, halfwidth=32, dtype=npdt)
    for i in range(nplant):
        row = 7 + 42 * i
        ks = np.arange(A.row_ptr[row], A.row_ptr[row + 1])
        A.val[ks[A.col[ks] == row][0]] += 4 + 2 * i
    return A


def dense(A):
    D = np.zeros((A.n, A.n))
    for row in range(A.n):
        s = slice(A.row_ptr[row], A.row_ptr[row + 1])
        D[row, A.col[s]] = A.val[s]
    return D


def f64(x):
    return np.asarray(x, np.float64)


def wanted(T, nkeep, which):
    """Eigenpairs of the projected matrix, the wanted end first."""
    ev, E = np.linalg.eigh(0.5 * (T + T.T))
    idx = np.arange(T.shape[0]) if which == "smallest" else np.arange(T.shape[0])[::-1]
    return ev[idx[:nkeep]], E[:, idx[:nkeep]]


def restated_cycles(mul, B, b, m, r, which, passes, npdt):
    """The NumPy restatement of the thick-restart loop in the solve's precision (sqrtm and
    the eigendecomposition of T by eigh in fp64; the basis, W and every product on them
    in npdt).  A generator: after every cycle it yields fp64 copies of P = [Q_0 .. Q_{m-1}],
    the projected T and beta_m, then restarts keeping r blocks."""
    def sqrtm_pair(G):
        G = f64(G)
        w, U = np.linalg.eigh(0.5 * (G + G.T))
        w = np.abs(w)
        return ((U * np.sqrt(w)) @ U.T).astype(npdt), ((U / np.sqrt(w)) @ U.T).astype(npdt)

    Q, alpha, beta = [None] * m, [None] * m, [None] * (m + 1)

    def steps(W, j0, S=None):
        for j in range(j0, m):
            beta[j], bi = sqrtm_pair(W.T @ W)
            Q[j] = W @ bi
            W = mul(Q[j])
            if S is not None and j == j0:
                W = W - np.concatenate(Q[:j0], axis=1) @ S  # Y Sigma^T
            elif j:
                W = W - Q[j - 1] @ beta[j]
            a = W.T @ Q[j]
            alpha[j] = (0.5 * (a + a.T)).astype(npdt)
            W = W - Q[j] @ alpha[j]
            P = np.concatenate(Q[:j + 1], axis=1)
            for _ in range(passes):
                W = W - P @ (P.T @ W)
        beta[m] = sqrtm_pair(W.T @ W)[0]
        return W

    def tail(T, j0):
        for j in range(j0, m):
            T[j * b:(j + 1) * b, j * b:(j + 1) * b] = f64(alpha[j])
            if j > j0:
                T[(j - 1) * b:j * b, j * b:(j + 1) * b] = f64(beta[j])
                T[j * b:(j + 1) * b, (j - 1) * b:j * b] = f64(beta[j]).T

    W = steps(B.astype(npdt), 0)
    T = np.zeros((m * b, m * b))
    tail(T, 0)
    rb = r * b
    while True:
        P = f64(np.concatenate(Q, axis=1))
        bm = f64(beta[m])
        yield P, T.copy(), bm
        theta_k, Zk = wanted(T, rb, which)
        Sigma = bm @ Zk[-b:]
        Y = (P @ Zk).astype(npdt)
        for c in range(r):
            Q[c] = Y[:, c * b:(c + 1) * b]
        T = np.zeros((m * b, m * b))
        T[np.arange(rb), np.arange(rb)] = theta_k
        T[rb:rb + b, :rb] = Sigma
        T[:rb, rb:rb + b] = Sigma.T
        W = steps(W, r, S=Sigma.T.astype(npdt))
        tail(T, r)


def figures(D, P, T, bm, b, nev, which, ev):
    """What the tests measure from a basis, its projected matrix and beta_m (fp64 copies)."""
    theta, S = wanted(T, nev, which)
    resid = np.linalg.norm(bm @ S[-b:], axis=0)
    X = P @ S
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    ends = ev[:nev] if which == "smallest" else ev[::-1][:nev]
    scale = float(np.abs(np.linalg.eigvalsh(0.5 * (T + T.T))).max())  # max|theta| over all of T: the stop test's scale
    return dict(scale=scale, theta=theta, resid=resid, true=true, gap=float(np.abs(true - resid).max()),
                orth=float(np.abs(P.T @ P - np.eye(P.shape[1])).max()), dT=float(np.abs(P.T @ D @ P - T).max()),
                xo=float(np.abs(X.T @ X - np.eye(nev)).max()), ritz_err=float(np.abs(theta - ends).max()))


CASES = {  # name: (n, b, m, r, nev, which, dtype, tol, planted rows)
    "b16": (1024, 16, 6, 2, 24, "largest", "f64", 1e-10, 24),
    "b5": (777, 5, 12, 5, 13, "largest", "f64", 1e-10, 8),
    "b16s": (1024, 16, 8, 3, 16, "smallest", "f64", 1e-8, 24),
    "b32f": (1024, 32, 4, 1, 24, "largest", "f32", 2e-5, 24),
}
LC = 5


class Problem:
    pass


_cache = {}


def problem(lz, torch, name):
    """The operator, its dense copy and spectrum, the start block, and the restatement run
    to convergence (figures after every cycle), once per shape."""
    if name in _cache:
        return _cache[name]
    n, b, m, r, nev, which, dt, tol, npl = CASES[name]
    s = Problem()
    s.npdt, s.tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    s.eps = EPS64 if dt == "f64" else EPS32
    s.A = planted(lz, n, npl, s.npdt)
    s.D = dense(s.A)
    s.ev = np.linalg.eigvalsh(s.D)
    s.norm1 = float(np.abs(s.D).sum(axis=0).max())
    s.Bh = lz.uniform_B(n, b, dtype=s.npdt)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.vs = -(-n * b // 4) * 4  # a multiple of 16 bytes in both precisions (777 * 5 is odd)
    Dp = s.D.astype(s.npdt)
    s.ref = []  # the restatement's figures after cycle 1, 2, ... up to convergence
    for P, T, bm in restated_cycles(lambda Q: Dp @ Q, s.Bh, b, m, r, which, 2, s.npdt):
        s.ref.append(figures(s.D, P, T, bm, b, nev, which, s.ev))
        f = s.ref[-1]
        if f["resid"].max() <= tol * f["scale"]:
            break
        assert len(s.ref) < 40, "the restatement does not converge"
    s.cycles_ref = len(s.ref)
    _cache[name] = s
    return s


def host_panel(V, m, vs, n, b):
    return f64(V.view(m, vs)[:, :n * b].reshape(m, n, b).permute(1, 0, 2).reshape(n, m * b).cpu().numpy())


@pytest.mark.parametrize("name", list(CASES))
def test_resume(lz, handle, torch_cuda, name):
    """One cycle, the host restart, the compress, one resumed cycle: the basis is orthonormal,
    P^T A P (lz_csr_spmm + lz_panel_gram) is the T of lzh_restart_coeffs + lzh_restart_fill
    -- a transposed or misplaced Sigma fails here -- the residual estimates are the true
    residual norms, q is row lc of every block, and alpha / beta of the kept part are not
    written."""
    torch = torch_cuda
    n, b, m, r, nev, which, dt, tol, _ = CASES[name]
    s = problem(lz, torch, name)
    vs = s.vs
    kw = dict(dtype=s.tdt, device="cuda")
    V = torch.full((m * vs,), float("nan"), **kw)
    W = torch.empty(n, b, **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(s.Ad, torch.from_numpy(s.Bh).cuda(), m, LC, q, al, be, V, vs, W, passes=2)
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.Assemble_T(m, b, alpha, beta)
    theta_k, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], which)
    handle.panel_compress(V, vs, m, r, torch.from_numpy(Z).to(**kw), n=n)
    qh = f64(q.cpu().numpy()) @ Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)  # row lc of Y, on the host
    q[:r * b] = torch.from_numpy(qh).to(**kw)
    q0, al0, be0 = q.clone(), al.clone(), be.clone()
    handle.block_lanczos_reorth_resume(s.Ad, r, m, LC, torch.from_numpy(sigma).to(**kw), q, al, be, V, vs, W,
                                       passes=2)
    assert torch.equal(al[:r], al0[:r]) and torch.equal(be[:r], be0[:r]) and torch.equal(q[:r * b], q0[:r * b])
    alpha, beta = f64(al.cpu().numpy()), f64(be.cpu().numpy())
    T = lz.restart_fill(r, m, b, alpha, beta, Tn)
    P = host_panel(V, m, vs, n, b)
    assert np.isfinite(P).all()
    ref = s.ref[1]  # the restatement after its second cycle
    orth = float(np.abs(P.T @ P - np.eye(m * b)).max())
    print(f"{name}: after one restart max|P^T P - I| = {orth:.3e} (restatement {ref['orth']:.3e})")
    assert orth <= 100 * ref["orth"]
    # T_proj, block column by block column: Y = A Q_j, then [Q_i^T Y for all i]
    Y = torch.empty(n, b, **kw)
    C = torch.empty(m, b, b, **kw)
    Tp = np.zeros((m * b, m * b))
    for j in range(m):
        handle.spmm(s.Ad, V[j * vs:j * vs + n * b].view(n, b), Y)
        handle.panel_gram(V, vs, m, Y, C)
        Tp[:, j * b:(j + 1) * b] = f64(C.cpu().numpy()).reshape(m * b, b)
    dT = float(np.abs(Tp - T).max())
    dT_bound = 1e-10 if dt == "f64" else 100 * ref["dT"]
    print(f"{name}: max|P^T A P - T| = {dT:.3e} (bound {dT_bound:.3e}, restatement {ref['dT']:.3e})")
    assert dT <= dT_bound
    theta, S, resid = lz.ritz_pairs_dense(m, b, T, beta[m], nev, which)
    X = P @ S
    true = np.linalg.norm(s.D @ X - X * theta, axis=0)
    gap = float(np.abs(true - resid).max())
    gap_bound = 1e-10 * s.norm1 if dt == "f64" else 100 * ref["gap"]
    print(f"{name}: residual norms vs estimate: max gap {gap:.3e} (bound {gap_bound:.3e}, restatement {ref['gap']:.3e})")
    assert gap <= gap_bound
    qd = f64(q.cpu().numpy())
    assert np.array_equal(qd[r * b:], P[LC, r * b:]), "q = row lc of every new Q_j"
    dq = float(np.abs(qd[:r * b] - P[LC, :r * b]).max())
    print(f"{name}: kept blocks: max|q - Y[lc]| = {dq:.3e} (bound {8 * m * b * s.eps:.3e})")
    assert dq <= 8 * m * b * s.eps


def run_eigsh(lz, handle, torch, name, s):
    n, b, m, r, nev, which, dt, tol, _ = CASES[name]
    return handle.eigsh(s.Ad, nev, which=which, b=b, m=m, keep=r, tol=tol, max_cycles=2 * s.cycles_ref,
                        B=torch.from_numpy(s.Bh).cuda(), lc=LC, passes=2)


@pytest.mark.parametrize("name", list(CASES))
def test_eigsh(lz, handle, torch_cuda, name):
    """The driver converges within twice the restatement's cycle count (a cap, so that a run
    that does not converge cannot pass as slow), to the outermost eigenvalues in order -- a
    ghost or a missed eigenvalue breaks the order -- with orthonormal Ritz vectors in the
    first blocks of the same panel, and it is bitwise reproducible."""
    torch = torch_cuda
    n, b, m, r, nev, which, dt, tol, _ = CASES[name]
    s = problem(lz, torch, name)
    ref = s.ref[-1]
    out = run_eigsh(lz, handle, torch, name, s)
    print(f"{name}: device {out['cycles']} cycles, {out['n_spmm']} SpMMs (restatement {s.cycles_ref} cycles, "
          f"{m + (s.cycles_ref - 1) * (m - r)} SpMMs); per-cycle max wanted residual "
          + " ".join(f"{x:.1e}" for x in out["history"]))
    assert out["converged"] and out["cycles"] <= 2 * s.cycles_ref
    assert out["n_spmm"] == m + (out["cycles"] - 1) * (m - r) and len(out["history"]) == out["cycles"]
    theta, vs = out["theta"], out["vstride"]
    nch = -(-nev // b)
    Xp = host_panel(out["V"][:nch * vs], nch, vs, n, b)
    assert np.isfinite(Xp).all() and (Xp[:, nev:] == 0).all(), "the last block is zero-padded"
    X = Xp[:, :nev]
    ends = s.ev[:nev] if which == "smallest" else s.ev[::-1][:nev]
    err = np.abs(theta - ends)
    true = np.linalg.norm(s.D @ X - X * theta, axis=0)
    xo = float(np.abs(X.T @ X - np.eye(nev)).max())
    print(f"{name}: max Ritz error {err.max():.3e}, max true residual {true.max():.3e}, estimate "
          f"{out['resid'].max():.3e}, max|X^T X - I| {xo:.3e} (restatement: {ref['ritz_err']:.3e}, "
          f"{ref['true'].max():.3e}, {ref['resid'].max():.3e}, {ref['xo']:.3e})")
    if dt == "f64":
        bound = tol * out["scale"] + 1e-10 * s.norm1
        assert (err <= bound).all()
        assert (true <= bound).all()
    else:
        assert err.max() <= 100 * ref["ritz_err"]
        assert true.max() <= 100 * ref["true"].max()
    assert xo <= 100 * ref["xo"]
    out2 = run_eigsh(lz, handle, torch, name, s)
    assert out2["cycles"] == out["cycles"] and np.array_equal(out2["theta"], theta)
    assert np.array_equal(out2["resid"], out["resid"]) and torch.equal(out2["V"][:nch * vs], out["V"][:nch * vs])


def test_single_solve_does_not_converge(lz, torch_cuda):
    """At the first shape a single m = 6 solve does not meet the tolerance for 24 pairs (a
    statement about the operator, made on the restatement's first cycle): the restart is
    what converges them in six blocks."""
    n, b, m, r, nev, which, dt, tol, _ = CASES["b16"]
    s = problem(lz, torch_cuda, "b16")
    first = s.ref[0]
    print(f"m = 6 single solve: max wanted residual {first['resid'].max():.3e}, true {first['true'].max():.3e}")
    assert first["resid"].max() > tol * first["scale"]
    assert first["true"].max() > tol * first["scale"] + 1e-10 * s.norm1
    assert s.cycles_ref > 1


def test_eigsh_max_cycles_returns_unconverged(lz, handle, torch_cuda):
    s = problem(lz, torch_cuda, "b16")
    n, b, m, r, nev, which, dt, tol, _ = CASES["b16"]
    out = handle.eigsh(s.Ad, nev, which=which, b=b, m=m, keep=r, tol=tol, max_cycles=2,
                       B=torch_cuda.from_numpy(s.Bh).cuda(), lc=LC)
    assert out["converged"] is False and out["cycles"] == 2 and len(out["history"]) == 2


def test_eigsh_defaults(lz, handle, torch_cuda):
    """keep, m and B left to the driver: nev = 8 at b = 16 gives keep = 2 (2 * 16 >= 8 + 16)
    and m = 4; the 8 largest eigenvalues of the planted operator come out in order."""
    s = problem(lz, torch_cuda, "b16")
    tol = 1e-9
    out = handle.eigsh(s.Ad, 8, tol=tol, lc=LC)
    print(f"defaults: {out['cycles']} cycles, {out['n_spmm']} SpMMs, max estimate {out['resid'].max():.3e}")
    assert out["converged"] and out["n_spmm"] == 4 + (out["cycles"] - 1) * 2
    assert (np.abs(out["theta"] - s.ev[::-1][:8]) <= tol * out["scale"] + 1e-10 * s.norm1).all()


def test_argument_checks(lz, handle, torch_cuda):
    torch = torch_cuda
    L, kw = handle.L, dict(dtype=torch.float64, device="cuda")
    n, b, k = 64, 16, 3
    V, W = torch.zeros(20 * n * b, **kw), torch.zeros(n, b, **kw)
    Z, sg = torch.zeros(17, 20, b, b, **kw), torch.zeros(k, b, b, **kw)
    p = lambda t: t.data_ptr()

    def is_arg_error(rc):
        assert rc == -1 and L.lz_last_error(), rc  # LZ_E_ARG with a message

    comp = lambda k_, r_, vs_=n * b, z_=p(Z), b_=b: L.lz_panel_compress(handle.ptr, n, b_, k_, r_, lz.LZ_F64, p(V), vs_, z_)
    is_arg_error(comp(k, 0))
    is_arg_error(comp(20, 17))      # r > 16
    is_arg_error(comp(k, k + 1))    # r > k
    is_arg_error(comp(65, 2))
    is_arg_error(comp(k, 2, z_=None))
    is_arg_error(comp(k, 2, vs_=n * b - 2))
    is_arg_error(comp(k, 2, vs_=n * 33 + 1, b_=33))
    A = lz.CsrDevice.from_host(lz.gen_banded(n, 5, 8))
    q, al, be = torch.zeros(k * b, **kw), torch.zeros(k, b, b, **kw), torch.zeros(k + 1, b, b, **kw)
    res = lambda r_, m_, vs_=n * b, s_=p(sg), passes=2: L.lz_block_lanczos_reorth_resume(
        handle.ptr, n, A.nnz, p(A.row_ptr), p(A.col), p(A.val), A.dtype, b, r_, m_, 5, s_, p(q), p(al), p(be), p(V),
        vs_, p(W), passes)
    is_arg_error(res(0, k))
    is_arg_error(res(k, k))         # r >= m
    is_arg_error(res(1, 65))
    is_arg_error(res(1, k, s_=None))
    is_arg_error(res(1, k, vs_=n * b - 2))
    is_arg_error(res(1, k, passes=3))
    with pytest.raises(lz.LanczosError, match="keep"):
        handle.eigsh(A, 20, b=b, m=4, keep=1)   # keep * b < nev
    with pytest.raises(lz.LanczosError, match="keep"):
        handle.eigsh(A, 8, b=b, m=2, keep=2)    # keep >= m
