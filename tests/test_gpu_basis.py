"""Kept Krylov basis: the two panel kernels (lz_panel_gram, lz_panel_apply), the
reorthogonalised solve (lz_block_lanczos_reorth) and Ritz vectors.

Panel kernels: inputs uniform in (-1, 1), references NumPy in fp64.
  fp64 tolerance  8 L eps64, the gamma_L bound of a length-L sum of products of
                  magnitude <= 1.  The Gram contracts over the n rows (L = n); the
                  apply contracts over the k b columns of the panel (L = k b, plus
                  one term for beta W).
  fp32 tolerance  4 eps32 sum|v||w| per entry (sums are fp64, rounded once).
Solver: the orthogonality bound is measured, not fixed: a NumPy restatement of the
same loop (eigh for the sqrtm) runs beside the device and the device may be at
most 100 x worse.  fp64 solves meet the issue's 1e-10 bounds; the fp32 solve, which
cannot, is held to 100 x its fp32 restatement's figures in the same way.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
G16, GGEN = 16, 4  # lz.PANEL_GROUP_16 / PANEL_GROUP_GEN (asserted below)

# (n, b, k, dtype, pad): every shape of the issue; the block-group boundary of
# both kernels (k = G, G + 1); pad = 32: vstride = n*b + 32 with NaN in the padding
PANEL_CASES = [
    (1, 16, 1, "f64", 0),
    (15, 16, 3, "f64", 0),
    (17, 16, 2, "f64", 32),
    (4099, 16, 1, "f64", 0),
    (4099, 16, G16, "f64", 0),
    (4099, 16, G16 + 1, "f64", 32),
    (4099, 16, 64, "f64", 0),
    (1000, 5, 7, "f64", 32),
    (1000, 32, 3, "f32", 0),
    (1000, 16, 4, "f32", 32),
]
IDS = ["n%d-b%d-k%d-%s-pad%d" % c for c in PANEL_CASES]


def test_group_constants(lz):
    assert (lz.PANEL_GROUP_16, lz.PANEL_GROUP_GEN, lz.PANEL_MAX_BLOCKS) == (G16, GGEN, 64)


def make_panel(torch, n, b, k, dt, pad, seed):
    """Host fp64 copies (of the stored values) and device buffers of a k-block panel, W and S."""
    npdt = np.float64 if dt == "f64" else np.float32
    rng = np.random.default_rng(seed)
    Vh = rng.uniform(-1, 1, (k, n, b)).astype(npdt)
    Wh = rng.uniform(-1, 1, (n, b)).astype(npdt)
    Sh = rng.uniform(-1, 1, (k, b, b)).astype(npdt)
    vstride = n * b + pad
    buf = np.full(k * vstride, np.nan, npdt)
    for j in range(k):
        buf[j * vstride:j * vstride + n * b] = Vh[j].ravel()
    dev = lambda a: torch.from_numpy(a).cuda()
    return (Vh.astype(np.float64), Wh.astype(np.float64), Sh.astype(np.float64), dev(buf), dev(Wh), dev(Sh), vstride)


def expect_ids(lz, b, dt):
    mf = b == 16 and dt == "f64"
    return (lz.LZ_K_PGRAM16 if mf else lz.LZ_K_PGRAM_GEN, lz.LZ_K_PAPPLY16 if mf else lz.LZ_K_PAPPLY_GEN)


@pytest.mark.parametrize("n,b,k,dt,pad", PANEL_CASES, ids=IDS)
def test_panel_gram(lz, handle, torch_cuda, n, b, k, dt, pad):
    torch = torch_cuda
    Vh, Wh, _, V, W, _, vs = make_panel(torch, n, b, k, dt, pad, 100 + n + k)
    C = torch.full((k, b, b), float("nan"), dtype=W.dtype, device="cuda")
    handle.panel_gram(V, vs, k, W, C)
    assert handle.last_kernel()[1] == expect_ids(lz, b, dt)[0]
    got = C.cpu().numpy().astype(np.float64)
    ref = np.einsum("jri,rc->jic", Vh, Wh)
    err = np.abs(got - ref)
    if dt == "f64":
        tol = 8 * n * EPS64
        print(f"panel_gram {n}x{b} k={k}: max err {err.max():.3e} (tol {tol:.3e})")
        assert np.isfinite(got).all() and err.max() <= tol
    else:
        bound = 4 * EPS32 * np.einsum("jri,rc->jic", np.abs(Vh), np.abs(Wh))
        print(f"panel_gram {n}x{b} k={k} fp32: max err/bound {(err / bound).max():.3e}")
        assert np.isfinite(got).all() and (err <= bound).all()
    C2 = torch.full_like(C, float("nan"))
    handle.panel_gram(V, vs, k, W, C2)
    assert torch.equal(C, C2), "two identical calls must agree bitwise"


@pytest.mark.parametrize("n,b,k,dt,pad", PANEL_CASES, ids=IDS)
def test_panel_apply(lz, handle, torch_cuda, n, b, k, dt, pad):
    torch = torch_cuda
    Vh, Wh, Sh, V, W0, S, vs = make_panel(torch, n, b, k, dt, pad, 200 + n + k)
    prod = np.einsum("jri,jic->rc", Vh, Sh)
    aprod = np.einsum("jri,jic->rc", np.abs(Vh), np.abs(Sh))

    def check(got, ref, mag, what):
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all(), what + ": NaN / Inf in the output"
        if dt == "f64":
            tol = 8 * (k * b + 1) * EPS64
            print(f"panel_apply {what} {n}x{b} k={k}: max err {err.max():.3e} (tol {tol:.3e})")
            assert err.max() <= tol
        else:
            print(f"panel_apply {what} {n}x{b} k={k} fp32: max err/bound {(err / (4 * EPS32 * mag)).max():.3e}")
            assert (err <= 4 * EPS32 * mag).all()

    # beta = 0 never reads W: a NaN-filled W must not reach the output
    W = torch.full_like(W0, float("nan"))
    handle.panel_apply(0.0, 1.0, V, vs, k, S, W)
    assert handle.last_kernel()[1] == expect_ids(lz, b, dt)[1]
    check(W.cpu().numpy(), prod, aprod, "beta=0")
    # the reorthogonalisation's update W -= V S
    W1 = W0.clone()
    handle.panel_apply(1.0, -1.0, V, vs, k, S, W1)
    check(W1.cpu().numpy(), Wh - prod, np.abs(Wh) + aprod, "beta=1 alpha=-1")
    W2 = W0.clone()
    handle.panel_apply(1.0, -1.0, V, vs, k, S, W2)
    assert torch.equal(W1, W2), "two identical calls must agree bitwise"


def test_panel_past_4gib(lz, handle, torch_cuda):
    """A 4.4 GB panel: every block past the seventh starts beyond a 32-bit byte offset.
    Filled on the device; reference torch fp64 matmul on the device, block by block."""
    torch = torch_cuda
    n, b, k = (1 << 20) + 3, 16, 33
    vs = n * b
    assert k * vs * 8 > (1 << 32)
    g = torch.Generator(device="cuda").manual_seed(4242)
    V = torch.rand(k * vs, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    W = torch.rand(n, b, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    S = torch.rand(k, b, b, dtype=torch.float64, device="cuda", generator=g).mul_(2).sub_(1)
    Vv = V.view(k, n, b)
    C = torch.empty(k, b, b, dtype=torch.float64, device="cuda")
    handle.panel_gram(V, vs, k, W, C)
    assert handle.last_kernel()[1] == lz.LZ_K_PGRAM16
    Cref = torch.stack([Vv[j].T @ W for j in range(k)])
    eg = float((C - Cref).abs().max())
    print(f"4 GiB panel_gram: max err {eg:.3e} (tol {8 * n * EPS64:.3e})")
    assert eg <= 8 * n * EPS64
    Wref = W.clone()
    for j in range(k):
        Wref.addmm_(Vv[j], S[j], alpha=-1.0)
    handle.panel_apply(1.0, -1.0, V, vs, k, S, W)
    assert handle.last_kernel()[1] == lz.LZ_K_PAPPLY16
    ea = float((W - Wref).abs().max())
    print(f"4 GiB panel_apply: max err {ea:.3e} (tol {8 * (k * b + 1) * EPS64:.3e})")
    assert ea <= 8 * (k * b + 1) * EPS64


# ------------------------------------------------------------------ solver
def planted(lz, n, nplant, npdt):
    """gen_banded(n, 9 nnz/row, halfwidth 32) with 4 + 2i added to the diagonal of row 7 + 42i."""
    A = lz.gen_banded(n, nnz_per_row=9, halfwidth=32, dtype=npdt)
    for i in range(nplant):
        r = 7 + 42 * i
        ks = np.arange(A.row_ptr[r], A.row_ptr[r + 1])
        A.val[ks[A.col[ks] == r][0]] += 4 + 2 * i
    return A


def dense(A):
    D = np.zeros((A.n, A.n))
    for r in range(A.n):
        s = slice(A.row_ptr[r], A.row_ptr[r + 1])
        D[r, A.col[s]] = A.val[s]
    return D


def csr_mul(A, npdt):
    """Q -> A Q from the CSR arrays (every row has its diagonal entry, so reduceat is safe)."""
    val, col, starts = A.val.astype(npdt), A.col, A.row_ptr[:-1]
    return lambda Q: np.add.reduceat(val[:, None] * Q[col], starts, axis=0).astype(npdt)


def restated(mul, B, m, passes, npdt):
    """The NumPy restatement of lz_block_lanczos_reorth's loop in the solve's precision
    (sqrtm by eigh, rounded to that precision): P (fp64 copy), alpha, beta (m + 1 blocks)."""
    B = B.astype(npdt)

    def sqrtm_pair(Gm):
        Gm = Gm.astype(np.float64)
        w, U = np.linalg.eigh(0.5 * (Gm + Gm.T))
        w = np.abs(w)
        return ((U * np.sqrt(w)) @ U.T).astype(npdt), ((U / np.sqrt(w)) @ U.T).astype(npdt)

    Q, alpha, beta = [], [], []
    W = B
    for j in range(m):
        be, bi = sqrtm_pair(W.T @ W)
        beta.append(be)
        Q.append(W @ bi)
        W = mul(Q[j])
        if j:
            W = W - Q[j - 1] @ be
        a = W.T @ Q[j]
        alpha.append((0.5 * (a + a.T)).astype(npdt))
        W = W - Q[j] @ alpha[j]
        P = np.concatenate(Q, axis=1)
        for _ in range(passes):
            W = W - P @ (P.T @ W)
    beta.append(sqrtm_pair(W.T @ W)[0])
    f64 = lambda x: np.asarray(x, np.float64)
    return f64(np.concatenate(Q, axis=1)), f64(alpha), f64(beta)


def orthogonality(P):
    return float(np.abs(P.T @ P - np.eye(P.shape[1])).max())


def figures(lz, D, ev, P, alpha, beta, m, b, nev=16):
    """What the solver tests measure, from a basis and its alpha / beta (all fp64 copies):
    Ritz-value errors and residual estimates of the nev largest pairs, the gap between true
    and estimated residual norms of X = P S, and max|P^T A P - Assemble_T|."""
    theta, S, resid = lz.ritz_pairs(m, b, alpha, beta, nev, "largest")
    X = P @ S
    true = np.linalg.norm(D @ X - X * theta, axis=0)
    T = lz.Assemble_T(m, b, alpha, beta)
    return dict(ritz_err=np.abs(theta - ev[::-1][:nev]), resid=resid, gap=float(np.abs(true - resid).max()),
                dT=float(np.abs(P.T @ D @ P - T).max()))


SOLVES = {  # name: (n, b, m, planted rows, dtype)
    "b16": (1024, 16, 20, 24, "f64"),
    "b5": (777, 5, 30, 8, "f64"),
    "b32f": (1024, 32, 8, 24, "f32"),
    "m1": (1024, 16, 1, 24, "f64"),
}


class Solve:
    pass


_cache = {}


def solved(lz, handle, torch, name):
    """One passes = 2 solve per shape, shared by the tests below (results on the host),
    and the NumPy restatement of the same solve with the same figures taken from it."""
    if name in _cache:
        return _cache[name]
    n, b, m, npl, dt = SOLVES[name]
    npdt, tdt = (np.float64, torch.float64) if dt == "f64" else (np.float32, torch.float32)
    s = Solve()
    s.n, s.b, s.m, s.dt, s.lc = n, b, m, dt, 5
    s.A = planted(lz, n, npl, npdt)
    s.D = dense(s.A)
    s.Bh = lz.uniform_B(n, b, dtype=npdt)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.vs = -(-n * b // 4) * 4  # a multiple of 16 bytes in both precisions (777 * 5 is odd)
    kw = dict(dtype=tdt, device="cuda")
    s.V = torch.full((m * s.vs,), float("nan"), **kw)
    s.W = torch.empty(n, b, **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(s.Ad, torch.from_numpy(s.Bh).cuda(), m, s.lc, q, al, be, s.V, s.vs, s.W, passes=2)
    s.q = q.cpu().numpy().astype(np.float64)
    s.alpha, s.beta = al.cpu().numpy().astype(np.float64), be.cpu().numpy().astype(np.float64)
    s.P = s.V.view(m, s.vs)[:, :n * b].reshape(m, n, b).permute(1, 0, 2).reshape(n, m * b).cpu().numpy().astype(np.float64)
    s.orth = orthogonality(s.P)
    s.T = lz.Assemble_T(m, b, s.alpha, s.beta)
    s.ev = np.linalg.eigvalsh(s.D)
    s.norm1 = float(np.abs(s.D).sum(axis=0).max())
    Dp = s.D.astype(npdt)
    Pr, ar, br = restated(lambda Q: Dp @ Q, s.Bh, m, 2, npdt)
    s.orth_ref = orthogonality(Pr)
    s.ref = figures(lz, s.D, s.ev, Pr, ar, br, m, b)
    _cache[name] = s
    return s


def bound(s, fp64_bound, ref_figure):
    """fp64 solves are held to the issue's bound.  1e-10 cannot be met in fp32, so an fp32
    solve is held, as for orthogonality, to 100 x what the fp32 NumPy restatement of the
    same solve gives for the same figure."""
    return fp64_bound if s.dt == "f64" else 100 * ref_figure


def test_passes0_matches_unfused_solve(lz, handle, torch_cuda):
    """passes = 0 is the plain recurrence: the unfused solve's kernels on the same data in
    the same order, so alpha, beta_0..beta_5 and q are the existing unfused solve's bit for
    bit (the issue asks for the 1e-10 parity bound; equality implies it)."""
    torch = torch_cuda
    n, b, m, lc = 1024, 16, 6, 5
    A = planted(lz, n, 24, np.float64)
    Ad = lz.CsrDevice.from_host(A)
    B = torch.from_numpy(lz.uniform_B(n, b)).cuda()
    q0, a0, b0 = lz.run_block_lanczos(handle, Ad, B, m, lc, fused=False)
    kw = dict(dtype=torch.float64, device="cuda")
    V, W = torch.empty(m * n * b, **kw), torch.empty(n, b, **kw)
    q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
    handle.block_lanczos_reorth(Ad, B, m, lc, q, al, be, V, n * b, W, passes=0)
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    print(f"passes=0 vs unfused: alpha {rel(al, a0):.2e} beta {rel(be[:m], b0[:m]):.2e} q {rel(q, q0):.2e}")
    assert rel(al, a0) <= 1e-10 and rel(be[:m], b0[:m]) <= 1e-10 and rel(q, q0) <= 1e-10
    assert torch.equal(al, a0) and torch.equal(be[:m], b0[:m]) and torch.equal(q, q0)
    # beta[m] is the true beta_m of the final residual, not the reference's inverse slot
    Wh = W.cpu().numpy()
    w, U = np.linalg.eigh(Wh.T @ Wh)
    bm = (U * np.sqrt(w)) @ U.T
    assert np.abs(be[m].cpu().numpy() - bm).max() <= 1e-10 * np.abs(bm).max()


@pytest.mark.parametrize("name", list(SOLVES))
def test_reorth_orthogonality(lz, handle, torch_cuda, name):
    """max|P^T P - I| of the kept basis at passes = 2: at most 100 x the NumPy restatement's
    (the margin covers the device's Newton-Schulz sqrtm and its summation order)."""
    s = solved(lz, handle, torch_cuda, name)
    print(f"{name}: device max|P^T P - I| = {s.orth:.3e}, restatement {s.orth_ref:.3e}")
    assert np.isfinite(s.P).all()
    assert s.orth <= 100 * s.orth_ref
    assert np.allclose(s.q.reshape(s.m, s.b), s.P[s.lc].reshape(s.m, s.b), rtol=0, atol=0), "q = row lc of every Q_j"


def test_reorth_long_solve_on_fresh_handle(lz, torch_cuda):
    """A long solve (m = 36: three block groups of the MFMA Gram, 256 workgroups' slabs) on a
    new handle.  The solve reserves the panel Gram's slab workspace for m blocks before its
    first step, so no step can grow it (and synchronise); the first solve on the fresh handle
    and a second one on the same handle give the same bits, and the basis is orthonormal to
    the measured bound."""
    torch = torch_cuda
    n, b, m = 8192, 16, 36
    A = planted(lz, n, 24, np.float64)
    Ad = lz.CsrDevice.from_host(A)
    Bh = lz.uniform_B(n, b)
    B = torch.from_numpy(Bh).cuda()
    kw = dict(dtype=torch.float64, device="cuda")
    h = lz.Handle(0)
    try:
        outs = []
        for _ in range(2):
            V, W = torch.full((m * n * b,), float("nan"), **kw), torch.empty(n, b, **kw)
            q, al, be = torch.zeros(m * b, **kw), torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
            h.block_lanczos_reorth(Ad, B, m, 5, q, al, be, V, n * b, W, passes=2)
            outs.append((V, W, q, al, be))
        torch.cuda.synchronize()
    finally:
        h.close()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    P = outs[0][0].view(m, n, b).permute(1, 0, 2).reshape(n, m * b)
    orth = float((P.T @ P - torch.eye(m * b, **kw)).abs().max())
    orth_ref = orthogonality(restated(csr_mul(A, np.float64), Bh, m, 2, np.float64)[0])
    print(f"n=8192 m=36 on a fresh handle: device max|P^T P - I| = {orth:.3e}, restatement {orth_ref:.3e}")
    assert orth <= 100 * orth_ref


@pytest.mark.parametrize("name", ["b16", "b5", "b32f"])
def test_reorth_ritz_values(lz, handle, torch_cuda, name):
    """No ghost copies: as many Ritz values above 3.5 as the dense operator has eigenvalues
    there.  At the issue's main shape the 16 largest equal the 16 largest eigenvalues to
    1e-10.  At b = 5, m = 30 the Krylov space has not converged that far (the NumPy
    restatement is 1.9e-4 off at the 16th; only the 8 planted outliers have converged), so
    there each of the 16 largest is held to the bound it must meet at any stage -- within
    its own residual estimate plus 1e-10 ||A||_1 of the matching eigenvalue -- and every one
    whose estimate is below 1e-10 to 1e-10 absolute.  The fp32 solve is held to 100 x the
    error of its fp32 NumPy restatement.  m = 1 is not in this test: its 16 Ritz values
    cannot count the operator's 29 eigenvalues above 3.5, and none has converged."""
    s = solved(lz, handle, torch_cuda, name)
    rv = lz.ritz_values(s.m, s.b, s.alpha, s.beta)
    assert int((rv > 3.5).sum()) == int((s.ev > 3.5).sum())
    theta, _, resid = lz.ritz_pairs(s.m, s.b, s.alpha, s.beta, 16, "largest")
    err = np.abs(theta - s.ev[::-1][:16])
    print(f"{name}: 16 largest Ritz values: max err {err.max():.3e}, max resid {resid.max():.3e}"
          f" (restatement: max err {s.ref['ritz_err'].max():.3e})")
    if name == "b16":
        assert err.max() <= 1e-10
    elif s.dt == "f64":
        assert (err <= resid + 1e-10 * s.norm1).all()
        conv = resid < 1e-10
        print(f"{name}: {int(conv.sum())} pairs with a residual estimate below 1e-10, max err {err[conv].max():.3e}")
        assert conv.any() and (err[conv] <= 1e-10).all()  # (7 of the 8 outliers in the restatement)
    else:
        assert err.max() <= 100 * s.ref["ritz_err"].max()


@pytest.mark.parametrize("name", list(SOLVES))
def test_reorth_ritz_vectors(lz, handle, torch_cuda, name):
    """X = P S for the 16 largest pairs: orthonormal to the measured bound, true residual
    norms equal to the estimate ||beta_m S_last|| to 1e-10 ||A||_1, and T_proj = P^T A P
    (lz_csr_spmm + lz_panel_gram) equal to Assemble_T to 1e-10: with passes = 2 nothing is
    left beyond the sub- and super-diagonal blocks.  (fp32: see `bound`.)"""
    torch = torch_cuda
    s = solved(lz, handle, torch, name)
    n, b, m, vs = s.n, s.b, s.m, s.vs
    nev = 16
    theta, S, resid = lz.ritz_pairs(m, b, s.alpha, s.beta, nev, "largest")
    nch = -(-nev // b)
    X = torch.full((nch, vs), float("nan"), dtype=s.V.dtype, device="cuda")
    handle.ritz_vectors(s.V, vs, S, X, n, b)
    Xh = X[:, :n * b].reshape(nch, n, b).permute(1, 0, 2).reshape(n, nch * b).cpu().numpy().astype(np.float64)
    assert np.isfinite(Xh).all()
    assert (Xh[:, nev:] == 0).all(), "a last chunk narrower than b is zero-padded"
    Xh = Xh[:, :nev]
    xo = float(np.abs(Xh.T @ Xh - np.eye(nev)).max())
    true = np.linalg.norm(s.D @ Xh - Xh * theta, axis=0)
    gap = float(np.abs(true - resid).max())
    gap_bound = bound(s, 1e-10 * s.norm1, s.ref["gap"])
    print(f"{name}: max|X^T X - I| {xo:.3e}; residual norms vs estimate: max gap {gap:.3e} "
          f"(bound {gap_bound:.3e}, restatement {s.ref['gap']:.3e}); largest residual {true.max():.3e}")
    assert xo <= 100 * s.orth_ref
    assert gap <= gap_bound
    # T_proj, block column by block column: Y = A Q_j, then [Q_i^T Y for all i]
    Y = torch.empty(n, b, dtype=s.V.dtype, device="cuda")
    C = torch.empty(m, b, b, dtype=s.V.dtype, device="cuda")
    Tp = np.zeros((m * b, m * b))
    for j in range(m):
        handle.spmm(s.Ad, s.V[j * vs:j * vs + n * b].view(n, b), Y)
        handle.panel_gram(s.V, vs, m, Y, C)
        Tp[:, j * b:(j + 1) * b] = C.cpu().numpy().astype(np.float64).reshape(m * b, b)
    dT = float(np.abs(Tp - s.T).max())
    dT_bound = bound(s, 1e-10, s.ref["dT"])
    print(f"{name}: max|P^T A P - Assemble_T| = {dT:.3e} (bound {dT_bound:.3e}, restatement {s.ref['dT']:.3e})")
    assert dT <= dT_bound


def test_argument_checks(lz, handle, torch_cuda):
    torch = torch_cuda
    L, kw = handle.L, dict(dtype=torch.float64, device="cuda")
    n, b, k = 64, 16, 2
    V, W, C = torch.zeros(k * n * b, **kw), torch.zeros(n, b, **kw), torch.zeros(k, b, b, **kw)
    p = lambda t: t.data_ptr()

    def is_arg_error(rc):
        assert rc == -1 and L.lz_last_error(), rc  # LZ_E_ARG with a message

    is_arg_error(L.lz_panel_gram(handle.ptr, n, b, k, lz.LZ_F64, p(V), n * b - 2, p(W), p(C)))
    is_arg_error(L.lz_panel_gram(handle.ptr, n, b, 0, lz.LZ_F64, p(V), n * b, p(W), p(C)))
    is_arg_error(L.lz_panel_gram(handle.ptr, n, 33, k, lz.LZ_F64, p(V), n * 33 + 1, p(W), p(C)))
    is_arg_error(L.lz_panel_apply(handle.ptr, n, b, 0, lz.LZ_F64, 1.0, -1.0, p(V), n * b, p(C), p(W)))
    is_arg_error(L.lz_panel_apply(handle.ptr, n, 33, k, lz.LZ_F64, 1.0, -1.0, p(V), n * 33 + 1, p(C), p(W)))
    is_arg_error(L.lz_panel_apply(handle.ptr, n, b, k, lz.LZ_F64, 1.0, -1.0, p(V), n * b - 2, p(C), p(W)))
    A = lz.CsrDevice.from_host(lz.gen_banded(n, 5, 8))
    B = torch.ones(n, b, **kw)
    q, al, be = torch.zeros(k * b, **kw), torch.zeros(k, b, b, **kw), torch.zeros(k + 1, b, b, **kw)
    for vstride, passes, bs, m in ((n * b, 3, b, k), (n * b - 2, 2, b, k), (n * 33 + 1, 2, 33, k), (n * b, 2, b, 0)):
        is_arg_error(L.lz_block_lanczos_reorth(handle.ptr, n, A.nnz, p(A.row_ptr), p(A.col), p(A.val), A.dtype, bs,
                                               m, 5, p(B), p(q), p(al), p(be), p(V), vstride, p(W), passes))
    with pytest.raises(lz.LanczosError, match="passes"):
        handle.block_lanczos_reorth(A, B, k, 5, q, al, be, V, n * b, W, passes=3)
