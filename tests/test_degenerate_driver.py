"""Never silently wrong: the eigen drivers (Handle.eigsh plain, filtered and sigma=, Handle.svds)
on repeated eigenvalues, clusters, rank-deficient start blocks, low-rank operators and exhausted
Krylov spaces, without a GPU -- test_restart_driver's stand-in handle at b = 4 (its sqrtm is the
device's: sqrt|lambda|, 1 / sqrt|lambda| with 1 / 0 = inf), test_shift_invert_driver's for sigma=.

The contract, checked here from the returned V, vstride, theta (and cols) alone on the dense fp64
operator D:

  1. only LanczosError leaves a driver; refusing a rank-deficient block it says "rank deficient"
     and names the start block or the cycle and step;
  2. converged = True means   max_i ||D x_i - theta_i x_i|| <= tol * scale + gap,
     max|X^T X - I| <= orth, and sorted theta within 2 (tol * scale + gap) of the wanted nev values
     of eigvalsh(D), sorted -- a missing or a doubled copy of a repeated eigenvalue fails this;
  3. converged = False comes with finite theta, resid and history.

gap and orth are 100 x the figures of the NumPy restatement (restated_cycles of test_gpu_restart,
in the solve's precision) at the cycle where it stops: gap its max|true residual - estimate|, orth
its max|X^T X - I|, neither taken below one rounding (eps * scale, eps: test_gpu_svds' convention;
a residual that is measured, not estimated, has no gap but that).  Where the start block is
deficient the restatement runs from uniform_B on the same operator, where the operator is
(low rank, decoupled) on the healthy operator of the same size and precision: the figures are
those of the arithmetic, not of the defect.  A healthy solve must converge within twice the
restatement's cycle count.

The helpers below are shared with test_gpu_degenerate.py, which runs the same families on the
device.
"""
import numpy as np
import pytest

from test_gpu_restart import dense, figures, planted, restated_cycles, wanted
from test_gpu_svds import svd_figures
from test_restart_driver import B_, LC, PASSES, columns, first, make_standin
from test_shift_invert_driver import make_inverse_standin

EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}


# ------------------------------------------------------------------ operators
def from_dense(lz, D, npdt=np.float64, keep=None):
    """CsrHost of the non-zeros of D (keep: a mask of further entries to store, zeros included)."""
    nz = (D != 0) if keep is None else ((D != 0) | keep)
    rp = np.zeros(D.shape[0] + 1, np.int64)
    np.cumsum(nz.sum(axis=1), out=rp[1:])
    return lz.CsrHost(D.shape[0], rp, np.nonzero(nz)[1].astype(np.int32), D[nz].astype(npdt))


def copies(lz, n0, k, nplant, npdt=np.float64, shift=0.0):
    """k bit-identical copies of planted(n0, nplant) on the diagonal (copy c plus shift * c * I),
    permuted symmetrically with a fixed seed: every eigenvalue has multiplicity exactly k (shift
    = 0).  Returns (CsrHost, the dense fp64 copy of the stored values)."""
    D0 = dense(planted(lz, n0, nplant, npdt))
    n = n0 * k
    D = np.zeros((n, n))
    for c in range(k):
        s = slice(c * n0, (c + 1) * n0)
        D[s, s] = D0 + shift * c * np.eye(n0)
    p = np.random.default_rng(20261021).permutation(n)
    D = D[np.ix_(p, p)]
    A = from_dense(lz, D, npdt)
    return A, dense(A)


def low_rank(lz, n, rank, npdt=np.float64, seed=40):
    """blockdiag(S, 0): S symmetric uniform(-1, 1) of `rank` rows, the other n - rank rows empty."""
    rng = np.random.default_rng(seed)
    S = rng.uniform(-1, 1, (rank, rank))
    D = np.zeros((n, n))
    D[:rank, :rank] = 0.5 * (S + S.T)
    A = from_dense(lz, D, npdt)
    return A, dense(A)


def two_blocks(lz, n, n1, npdt=np.float64):
    """blockdiag(A1, A2) of planted(n, 2) with the coupling between the first n1 rows and the
    rest removed: a start block that is zero outside A1's rows never leaves them."""
    D = dense(planted(lz, n, 2, npdt))
    D[:n1, n1:] = 0
    D[n1:, :n1] = 0
    A = from_dense(lz, D, npdt)
    return A, dense(A)


def deficient_blocks(B0):
    """The start blocks of D1 - D4 from a healthy one (columns 0, 1 and 3 exist at b >= 4)."""
    b = B0.shape[1]
    D1, D2, D4 = B0.copy(), B0.copy(), B0.copy()
    D1[:, 2] = 0
    D2[:, 1] = B0[:, 3]
    D3 = np.outer(B0[:, 0], np.arange(1, b + 1)).astype(B0.dtype)
    D4[:, 1] = B0[:, 3] * (1 + 1e-7) + 1e-7 * B0[:, 0]
    return {"D1": D1, "D2": D2, "D3": D3, "D4": D4}


# ------------------------------------------------------- restatement figures
def restate(D, B, b, m, r, nev, which, npdt, tol, mul=None, rr=None, cap=60):
    """restated_cycles on D (or on mul, a transformed operator) from B until its stop test; returns
    (cycles, gap, orth), gap and orth already x 100 (the module docstring).  rr = None:
    the plain solve (the estimate against tol * max|theta|).  rr = (select, scale): the filtered
    and sigma= solves' test -- Rayleigh-Ritz on D over the r * b kept Ritz vectors, the nev pairs
    select(lam) picks, residuals measured in npdt against tol * scale."""
    ev = np.linalg.eigvalsh(D)
    Dp = D.astype(npdt)
    cycles = 0
    for P, T, bm in restated_cycles(mul or (lambda Q: Dp @ Q), B, b, m, r, which, PASSES, npdt):
        cycles += 1
        if rr is None:
            f = figures(D, P, T, bm, b, nev, which, ev)
            done, gap, xo, scale = f["resid"].max() <= tol * f["scale"], f["gap"], f["xo"], f["scale"]
        else:
            select, scale = rr
            Y = (P @ wanted(T, r * b, which)[1]).astype(npdt)
            H = np.asarray(Y.T @ (Dp @ Y), np.float64)
            lam, C = np.linalg.eigh(0.5 * (H + H.T))
            sel = select(lam)[:nev]
            X = (Y @ C[:, sel].astype(npdt))
            claimed = np.linalg.norm(np.asarray(Dp @ X - X * lam[sel].astype(npdt), np.float64), axis=0)
            X64 = np.asarray(X, np.float64)
            true = np.linalg.norm(D @ X64 - X64 * lam[sel], axis=0)
            done, gap = claimed.max() <= tol * scale, float(np.abs(true - claimed).max())
            xo = float(np.abs(X64.T @ X64 - np.eye(len(sel))).max())
        if done:
            return cycles, 100 * max(gap, EPS[npdt] * scale), 100 * max(xo, EPS[npdt])
        assert cycles < cap, "the restatement does not converge"


def restate_svds(S, B, b, m, r, k, npdt, tol, cap=60):
    """The same for svds on S (R x C): (cycles, gap, orth) under svds' stop ratio; gap in units
    of sigma (svd_figures: the true ||P^T y - sigma x|| against est / sigma)."""
    Pd = S if S.shape[1] <= S.shape[0] else S.T
    Pp = Pd.astype(npdt)
    sd = np.linalg.svd(S, compute_uv=False)
    cycles = 0
    for Q, T, bm in restated_cycles(lambda Q: Pp.T @ (Pp @ Q), B, b, m, r, "largest", PASSES, npdt):
        cycles += 1
        f = svd_figures(Pd, Q, T, bm, b, k, EPS[npdt], sd)
        if f["ratio"] <= tol:
            return cycles, 100 * max(f["gap"], EPS[npdt] * sd[0]), 100 * max(f["xo"], f["yo"], EPS[npdt])
        assert cycles < cap, "the restatement does not converge"


def cheb_dense(D, filt):
    """p(D) of eigsh's filter = (degree, lo, hi, ref), dense: T_d((x - c0) / e) / T_d((ref - c0) / e)."""
    degree, lo, hi, ref = filt
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    w, U = np.linalg.eigh(D)
    cheb = np.polynomial.chebyshev.Chebyshev.basis(degree)
    return (U * (cheb((w - c0) / e) / cheb((ref - c0) / e))) @ U.T


# -------------------------------------------------------------- the contract
def is_finite(out, keys=("theta", "resid", "history")):
    for key in keys:
        assert np.isfinite(np.asarray(out[key], np.float64)).all(), f"{key} is not finite"


def verify_eig(name, D, X, theta, want, tol, scale, gap, orth):
    """Contract item 2 on the dense fp64 operator: X (n, nev) fp64 from the returned panel."""
    nev = len(want)
    assert X.shape[1] == nev == len(theta) and np.isfinite(X).all()
    true = np.linalg.norm(D @ X - X * theta, axis=0).max()
    xo = np.abs(X.T @ X - np.eye(nev)).max()
    err = np.abs(np.sort(theta) - np.sort(want)).max()
    bound = tol * scale + gap
    print(f"{name}: true residual {true:.3e} (bound {bound:.3e}), max|X^T X - I| {xo:.3e} (bound {orth:.3e}), "
          f"max|theta - eigvalsh| {err:.3e} (bound {2 * bound:.3e})")
    assert true <= bound, "a converged result whose residual on A is not small"
    assert xo <= orth
    assert err <= 2 * bound, "a missing or doubled eigenvalue"


def verify_svd(name, S, U, V, s, tol, gap, orth):
    k = len(s)
    sd = np.linalg.svd(S, compute_uv=False)
    left = np.linalg.norm(S.T @ U - V * s, axis=0).max()
    right = np.linalg.norm(S @ V - U * s, axis=0).max()
    uo, vo = np.abs(U.T @ U - np.eye(k)).max(), np.abs(V.T @ V - np.eye(k)).max()
    err = np.abs(np.sort(s) - np.sort(sd[:k])).max()
    bound = tol * sd[0] + gap
    print(f"{name}: residuals {left:.3e} {right:.3e} (bound {bound:.3e}), orthogonality {uo:.3e} {vo:.3e} (bound "
          f"{orth:.3e}), max|s - svd| {err:.3e} (bound {2 * bound:.3e})")
    assert max(left, right) <= bound, "a converged result whose residual on A is not small"
    assert max(uo, vo) <= orth
    assert err <= 2 * bound, "a missing or doubled singular value"


def ends(ev, nev, which="largest", sigma=None):
    if sigma is not None:
        return ev[np.argsort(np.abs(ev - sigma), kind="stable")[:nev]]
    return ev[:nev] if which == "smallest" else ev[::-1][:nev]


def never_silently_wrong(lz, name, solve, check, must_raise=False, finite=("theta", "resid", "history")):
    """Contract items 1 - 3 around solve(): a LanczosError is an accepted outcome (the required one
    with must_raise, and then it says "rank deficient" and where), any other exception is not; a
    converged result goes through check(out), an unconverged one must be finite.  Returns the
    outcome as a string."""
    try:
        with np.errstate(all="ignore"):
            out = solve()
    except lz.LanczosError as e:
        print(f"{name}: LanczosError: {e}")
        if must_raise:
            assert "rank deficient" in str(e) and ("start block" in str(e) or ("cycle" in str(e) and "step" in str(e)))
        return "raised"
    assert not must_raise, f"{name}: a rank-deficient block was not refused"
    if out["converged"]:
        check(out)
        return "converged"
    is_finite(out, finite)
    print(f"{name}: converged = False after {out['cycles']} cycles")
    return "not converged"


# ------------------------------------------------------- the stand-in at b = 4
M_, KEEP, NEV, TOL = 6, 2, 4, 1e-10
ARGS = dict(b=B_, m=M_, keep=KEEP, tol=TOL, lc=LC, passes=PASSES)


@pytest.fixture(scope="module")
def standin(lz):
    Handle, Csr = make_inverse_standin(lz)
    return Handle, lambda A, n_cols=None: Csr(A.n, n_cols or A.n, A.row_ptr, A.col, A.val)


def panel_columns(out, n, nev, key="V", stride="vstride"):
    X = columns(out[key], out[stride], n, -(-nev // B_))
    return X[:, out["cols"]] if "cols" in out else X[:, :nev]


def tensor(B):
    import torch
    return torch.from_numpy(np.ascontiguousarray(B))


HEALTHY = {  # name: (n0, copies, planted rows, shift, which, nev)
    "double": (96, 2, 2, 0.0, "largest", 4),
    "multiplicity-b": (64, 4, 1, 0.0, "largest", 4),
    "cluster-3e-9": (64, 4, 1, 1e-9, "largest", 4),
    "double-smallest": (96, 2, 2, 0.0, "smallest", 4),
}


@pytest.mark.parametrize("name", list(HEALTHY))
def test_repeated_eigenvalues_converge(lz, standin, name):
    Handle, dev = standin
    n0, k, npl, shift, which, nev = HEALTHY[name]
    A, D = copies(lz, n0, k, npl, shift=shift)
    B = lz.uniform_B(A.n, B_)
    cycles, gap, orth = restate(D, B, B_, M_, KEEP, nev, which, np.float64, TOL)
    out = Handle().eigsh(dev(A), nev, which=which, max_cycles=2 * cycles, B=tensor(B), **ARGS)
    print(f"{name}: {out['cycles']} cycles (restatement {cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale"}
    verify_eig(name, D, panel_columns(out, A.n, nev), out["theta"], ends(np.linalg.eigvalsh(D), nev, which), TOL,
               out["scale"], gap, orth)


@pytest.fixture(scope="module")
def lap20(lz):
    A = lz.gen_laplace2d(20, 20)
    D = dense(A)
    return A, D, np.linalg.eigvalsh(D)


def test_paired_eigenvalues_filtered(lz, standin, lap20):
    """The 20 x 20 Laplacian (eigenvalues in pairs), the six smallest through a degree-12 filter."""
    Handle, dev = standin
    A, D, ev = lap20
    B = lz.uniform_B(A.n, B_)
    args = {**ARGS, "tol": 1e-9}
    out = Handle().eigsh(dev(A), 6, which="smallest", filter_degree=12, max_cycles=40, B=tensor(B), **args)
    P = cheb_dense(D, out["filter"])
    cycles, gap, orth = restate(D, B, B_, M_, KEEP, 6, "largest", np.float64, 1e-9, mul=lambda Q: P @ Q,
                                rr=(lambda lam: np.argsort(lam, kind="stable"), out["scale"]))
    print(f"filtered: {out['cycles']} cycles (restatement {cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    verify_eig("filtered", D, panel_columns(out, A.n, 6), out["theta"], ev[:6], 1e-9, out["scale"], gap, orth)


def test_paired_eigenvalues_sigma(lz, standin, lap20):
    Handle, dev = standin
    A, D, ev = lap20
    B = lz.uniform_B(A.n, B_)
    Mi = np.linalg.inv(D)
    scale = max(abs(x) for x in lz.gershgorin(dev(A)))
    cycles, gap, orth = restate(D, B, B_, M_, KEEP, 6, "largest", np.float64, TOL, mul=lambda Q: Mi @ Q,
                                rr=(lambda lam: np.argsort(np.abs(lam), kind="stable"), scale))
    out = Handle().eigsh(dev(A), 6, sigma=0.0, inner="block", max_cycles=2 * cycles, B=tensor(B), **ARGS)
    print(f"sigma=0: {out['cycles']} cycles (restatement {cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    verify_eig("sigma=0", D, panel_columns(out, A.n, 6), out["theta"], ev[:6], TOL, out["scale"], gap, orth)


@pytest.mark.parametrize("shape", ["tall", "wide"])
def test_svds_repeated_singular_values(lz, standin, shape):
    """copies(96, 2, 2) stacked over a zero block (tall) and that transposed (wide)."""
    Handle, dev = standin
    A, D = copies(lz, 96, 2, 2)
    S = np.vstack([D, np.zeros((40, A.n))])
    S = S if shape == "tall" else np.ascontiguousarray(S.T)
    B = lz.uniform_B(A.n, B_)
    cycles, gap, orth = restate_svds(S, B, B_, M_, KEEP, NEV, np.float64, 1e-9)
    out = Handle().svds(dev(from_dense(lz, S), n_cols=S.shape[1]), NEV, max_cycles=2 * cycles, B=tensor(B),
                        **{**ARGS, "tol": 1e-9})
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    U = columns(out["U"], out["ustride"], S.shape[0], 1)[:, :NEV]
    V = columns(out["V"], out["vstride"], S.shape[1], 1)[:, :NEV]
    verify_svd(f"svds {shape}", S, U, V, out["s"], 1e-9, gap, orth)


# ------------------------------------------------------------------ deficient
@pytest.fixture(scope="module")
def plain(lz):
    """The healthy operator of the deficient start blocks: copies(96, 2, 2), its spectrum, and
    the restatement's figures from uniform_B."""
    A, D = copies(lz, 96, 2, 2)
    B0 = lz.uniform_B(A.n, B_)
    _, gap, orth = restate(D, B0, B_, M_, KEEP, NEV, "largest", np.float64, TOL)
    return A, D, np.linalg.eigvalsh(D), B0, gap, orth


@pytest.mark.parametrize("case", ["D1", "D2", "D3", "D4"])
def test_deficient_start_block(lz, standin, plain, case):
    """A zero column, a duplicated column, rank 1: refused after exactly one block_lanczos_reorth,
    no panel_compress and no resume.  D4 (duplicated to 1e-7): contract items 1 - 3."""
    Handle, dev = standin
    A, D, ev, B0, gap, orth = plain
    h = Handle()
    B = deficient_blocks(B0)[case]
    how = never_silently_wrong(
        lz, case, lambda: h.eigsh(dev(A), NEV, max_cycles=20, B=tensor(B), **ARGS),
        lambda out: verify_eig(case, D, panel_columns(out, A.n, NEV), out["theta"], ends(ev, NEV), TOL, out["scale"],
                               gap, orth), must_raise=case != "D4")
    if how == "raised":
        assert h.trace == [first(M_, A.n * B_)]


@pytest.mark.parametrize("case", ["D1", "D2"])
def test_svds_deficient_start_block(lz, standin, plain, case):
    Handle, dev = standin
    A, D, ev, B0, gap, orth = plain
    h = Handle()
    B = deficient_blocks(B0)[case]
    never_silently_wrong(lz, f"svds {case}", lambda: h.svds(dev(A), NEV, max_cycles=20, B=tensor(B), **ARGS), None,
                         must_raise=True)
    assert h.trace == [first(M_, A.n * B_, normal=True)]


def check_on(D, ev, n, nev, tol, gap, orth, name, which="largest", sigma=None):
    return lambda out: verify_eig(name, D, panel_columns(out, n, nev), out["theta"], ends(ev, nev, which, sigma), tol,
                                  out["scale"], gap, orth)


def test_d2_filtered_and_sigma(lz, standin, lap20, plain):
    """The duplicated column through the forms that measure their residuals on A: their
    Rayleigh-Ritz steps still assume an orthonormal panel."""
    Handle, dev = standin
    A, D, ev = lap20
    B0 = lz.uniform_B(A.n, B_)
    B = tensor(deficient_blocks(B0)["D2"])
    gap, orth = plain[4:]
    never_silently_wrong(lz, "D2 filtered", lambda: Handle().eigsh(dev(A), 6, which="smallest", filter_degree=12,
                                                                   max_cycles=12, B=B, **{**ARGS, "tol": 1e-9}),
                         check_on(D, ev, A.n, 6, 1e-9, gap, orth, "D2 filtered", "smallest"), must_raise=True)
    never_silently_wrong(lz, "D2 sigma", lambda: Handle().eigsh(dev(A), 6, sigma=0.0, inner="block", max_cycles=12, B=B,
                                                                **ARGS),
                         check_on(D, ev, A.n, 6, TOL, gap, orth, "D2 sigma", sigma=0.0), must_raise=True)


def test_d5_low_rank_operator(lz, standin, plain):
    """blockdiag(S10, 0) at n = 300: rank 10 < m b - b = 20, the Krylov space is exhausted in the
    first cycle; plain, filtered, sigma= and svds."""
    Handle, dev = standin
    A, D = low_rank(lz, 300, 10)
    ev = np.linalg.eigvalsh(D)
    gap, orth = plain[4:]
    for name, kw, which, sigma in [("D5", {}, "largest", None),
                                   ("D5 filtered", dict(which="smallest", filter_degree=8), "smallest", None),
                                   ("D5 sigma", dict(sigma=-0.5), "largest", -0.5)]:
        never_silently_wrong(lz, name, lambda: Handle().eigsh(dev(A), NEV, max_cycles=12, **{**ARGS, **kw}),
                             check_on(D, ev, A.n, NEV, TOL, gap, orth, name, which, sigma))

    def check(out):
        verify_svd("D5 svds", D, columns(out["U"], out["ustride"], A.n, 1)[:, :NEV],
                   columns(out["V"], out["vstride"], A.n, 1)[:, :NEV], out["s"], TOL, gap, orth)
    never_silently_wrong(lz, "D5 svds", lambda: Handle().svds(dev(A), NEV, max_cycles=12, **ARGS), check,
                         finite=("s", "resid", "est", "history"))


def test_d6_start_block_inside_an_invariant_subspace(lz, standin, plain):
    """blockdiag(A1 of 12 rows, A2), B zero outside A1's rows: A1's pairs are not A's outermost."""
    Handle, dev = standin
    A, D = two_blocks(lz, 192, 12)
    B = lz.uniform_B(A.n, B_)
    B[12:] = 0
    gap, orth = plain[4:]
    never_silently_wrong(lz, "D6", lambda: Handle().eigsh(dev(A), NEV, max_cycles=12, B=tensor(B), **ARGS),
                         check_on(D, np.linalg.eigvalsh(D), A.n, NEV, TOL, gap, orth, "D6"))


def test_d8_svds_few_rows(lz, standin, plain):
    """svds of a 90 x 60 matrix with 6 non-empty rows: rank 6 < m b - b."""
    Handle, dev = standin
    rng = np.random.default_rng(8)
    S = np.zeros((90, 60))
    S[::15] = rng.uniform(-1, 1, (6, 60))
    gap, orth = plain[4:]

    def check(out):
        verify_svd("D8", S, columns(out["U"], out["ustride"], 90, 1)[:, :NEV],
                   columns(out["V"], out["vstride"], 60, 1)[:, :NEV], out["s"], TOL, gap, orth)
    never_silently_wrong(lz, "D8", lambda: Handle().svds(dev(from_dense(lz, S), n_cols=60), NEV, max_cycles=12, **ARGS),
                         check, finite=("s", "resid", "est", "history"))


def test_d7_panel_wider_than_the_operator(lz, standin):
    """m * b > n is refused at argument time, before any device call: n = 20, b = 4, m = 6; svds
    by its Lanczos dimension min(R, C)."""
    Handle, dev = standin
    A, _ = copies(lz, 20, 1, 0)
    S = np.zeros((50, 20))
    S[np.arange(50), np.arange(50) % 20] = 1.0 + np.arange(50)
    h = Handle()
    for solve in (lambda: h.eigsh(dev(A), NEV, **ARGS),
                  lambda: h.eigsh(dev(A), NEV, filter_degree=8, **ARGS),
                  lambda: h.eigsh(dev(A), NEV, sigma=0.5, **ARGS),
                  lambda: h.eigsh_interval(dev(A), 0.1, 0.4, block=B_, m=M_, keep=KEEP),
                  lambda: h.svds(dev(from_dense(lz, S), n_cols=20), NEV, **ARGS),
                  lambda: h.svds(dev(from_dense(lz, np.ascontiguousarray(S.T)), n_cols=50), NEV, **ARGS)):
        with pytest.raises(lz.LanczosError, match=r"m \* b = 24 > n = 20"):
            solve()
    assert h.trace == []
