"""Handle.eigsh(sigma=...) without a GPU: test_restart_driver's stand-in handle, extended by the
inverse operator (a dense solve, optionally perturbed to a chosen relative residual) and NumPy
restatements of the panel kernels, spmm_resid and inverse_apply, runs the solver unchanged.

The operator is the 40 x 36 grid Laplacian (n = 1440).  sigma = 0 lies below the spectrum,
sigma = 0.5 inside it with 55 eigenvalues below and the nearest 3.5e-3 away, sigma = 4.0 in the
middle with a double eigenvalue nearest.  Checked per case: the call sequence, the counters,
theta against eigvalsh pair by pair within max(resid_i, 64 eps scale) (a symmetric matrix has
an eigenvalue within the residual norm of any Ritz value; the second term covers the rounding of
a residual measured near eps * scale), the order, and that sigma=None leaves the existing cases'
recorded traces as they were.

inner_tol_table() is the experiment behind INNER_TOL_FACTOR: run this file as a
script to print it.
"""
import numpy as np
import pytest

from test_restart_driver import B_, EIGSH, LC, PASSES, compress, make_standin, plain_trace, run_eigsh

NX, NY = 40, 36
M_, KEEP = 6, 2
SIGMAS = (0.0, 0.5, 4.0)
# exact-solve cycle counts at tol = 1e-10, (sigma, b) -> cycles: measured once with this file's
# stand-in (rel = 0) and asserted below, so a change in the driver that costs a cycle shows
EXACT_CYCLES = {(0.0, 4): 4, (0.5, 4): 5, (4.0, 4): 3, (0.0, 16): 4, (0.5, 16): 4, (4.0, 16): 4}
NEV = {4: 4, 16: 16}
EPS = float(np.finfo(np.float64).eps)


def make_inverse_standin(lz):
    """(InvHandle, DenseCsr): DenseHandle with inverse= on the two kept-basis solves."""
    import torch
    DenseHandle, DenseCsr = make_standin(lz)
    np_ = lambda t: t.numpy()
    inv_cache = {}

    def minv(A, sigma):
        key = (id(A), sigma)
        if key not in inv_cache:
            inv_cache[key] = (A, np.linalg.inv(A.dense - sigma * np.eye(A.n)))
        return inv_cache[key][1]

    class InvHandle(DenseHandle):
        """rel > 0: every inner solve X of M X = Q is returned as X + M^-1 E with E random and
        |E_c| = rel |Q_c|, so its relative residual is rel in every column."""

        def __init__(self, rel=0.0):
            super().__init__()
            self.rel, self.rng = rel, np.random.default_rng(5)

        def _inv(self, A, inverse):
            sigma, inner, tol, max_iter, info = inverse
            Mi = minv(A, sigma)

            def mul(Q):
                X = Mi @ Q
                if self.rel:
                    E = self.rng.standard_normal(Q.shape)
                    E *= self.rel * np.linalg.norm(Q, axis=0) / np.linalg.norm(E, axis=0)
                    X = X + Mi @ E
                res = np.linalg.norm(Q - (A.dense @ X - sigma * X), axis=0) / np.linalg.norm(Q, axis=0)
                info.solves += 1
                info.passes += 1
                info.n_spmm += 3  # (lz_minres_solve: passes + 2 + restarts)
                info.not_met += int((res > tol).sum())
                info.worst = max(info.worst, float(res.max()))
                return X
            return mul

        def block_lanczos_reorth(self, A, B, m, lc, q, alpha, beta, V, vstride, W, passes=2, filt=None, work=None,
                                 normal=None, inverse=None):
            if inverse is None:
                return super().block_lanczos_reorth(A, B, m, lc, q, alpha, beta, V, vstride, W, passes=passes,
                                                    filt=filt, work=work, normal=normal)
            self.trace.append(("block_lanczos_reorth", (m, lc, vstride, passes), "inverse", False))
            self.ops.append((inverse, work, None))
            W.copy_(B)
            self._steps(self._inv(A, inverse), 0, m, lc, None, q, alpha, beta, V, vstride, W, passes)

        def block_lanczos_reorth_resume(self, A, r, m, lc, sigma, q, alpha, beta, V, vstride, W, passes=2, filt=None,
                                        work=None, normal=None, inverse=None):
            if inverse is None:
                return super().block_lanczos_reorth_resume(A, r, m, lc, sigma, q, alpha, beta, V, vstride, W,
                                                           passes=passes, filt=filt, work=work, normal=normal)
            self.trace.append(("block_lanczos_reorth_resume", (r, m, lc, vstride, passes), "inverse", False))
            self.ops.append((inverse, work, None))
            b = W.shape[1]
            self._steps(self._inv(A, inverse), r, m, lc, np_(sigma).reshape(r * b, b), q, alpha, beta, V, vstride, W,
                        passes)

        def inverse_apply(self, A, inverse, X, Y, work):
            self.trace.append(("inverse_apply", tuple(X.shape), "inverse", False))
            np_(Y)[:] = self._inv(A, inverse)(np_(X))
            return Y

        @staticmethod
        def _blocks_of(V, vstride, k, n, b):
            Vh = np_(V)
            return [Vh[j * vstride:j * vstride + n * b].reshape(n, b) for j in range(k)]

        def panel_gram(self, V, vstride, k, W, C):
            n, b = W.shape
            self.trace.append(("panel_gram", (vstride, k, n), None, False))
            for j, Vj in enumerate(self._blocks_of(V, vstride, k, n, b)):
                np_(C)[j] = Vj.T @ np_(W)
            return C

        def panel_apply(self, beta, alpha, V, vstride, k, S, W):
            n, b = W.shape
            self.trace.append(("panel_apply", (vstride, k, n), None, False))
            acc = sum(Vj @ np_(S)[j] for j, Vj in enumerate(self._blocks_of(V, vstride, k, n, b)))
            np_(W)[:] = alpha * acc if beta == 0 else beta * np_(W) + alpha * acc
            return W

        def spmm_resid(self, A, X, theta, R, dots=None):
            n, b = X.shape
            self.trace.append(("spmm_resid", (n, b), None, False))
            np_(R)[:] = A.dense @ np_(X) - np_(X) * np_(theta)
            if dots is None:
                dots = torch.empty(2, b, dtype=torch.float64)
            d = np_(dots).reshape(2, b)
            d[0], d[1] = (np_(R) ** 2).sum(axis=0), (np_(R) * np_(X)).sum(axis=0)
            return R, dots.view(2, b)

    return InvHandle, DenseCsr


def laplace(lz, Csr):
    A = lz.gen_laplace2d(NX, NY)
    return Csr(A.n, A.n, A.row_ptr, A.col, A.val)


@pytest.fixture(scope="module")
def standin(lz):
    Handle, Csr = make_inverse_standin(lz)
    A = laplace(lz, Csr)
    return Handle, A, np.linalg.eigvalsh(A.dense)


def run(standin, sigma, b, rel=0.0, **over):
    Handle, A, _ = standin
    h = Handle(rel)
    args = dict(b=b, m=M_, keep=KEEP, lc=LC, passes=PASSES, sigma=sigma, max_cycles=2 * EXACT_CYCLES[(sigma, b)])
    args.update(over)
    return h, h.eigsh(A, NEV[b], **args)


@pytest.fixture(scope="module")
def solved(standin):
    """Every (sigma, b) case solved once with exact inner solves; the tests below only read."""
    return {(s, b): run(standin, s, b) for s in SIGMAS for b in (4, 16)}


def test_the_cases_are_what_the_docstring_says(standin):
    _, A, ev = standin
    assert A.n == NX * NY and ev[0] > 0.0
    assert (ev < 0.5).sum() == 55 and abs(np.abs(ev - 0.5).min() - 3.5e-3) < 1e-4
    near = np.sort(np.abs(ev - 4.0))
    assert near[1] - near[0] <= 64 * EPS * 8 and near[2] - near[1] > 1e-6  # the nearest eigenvalue is double


@pytest.mark.parametrize("b", [4, 16])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_trace_and_counters(standin, solved, sigma, b):
    _, A, _ = standin
    h, out = solved[(sigma, b)]
    n, nev, m, r = A.n, NEV[b], M_, KEEP
    cycles, nch, vs = out["cycles"], -(-NEV[b] // b), A.n * b
    print(f"sigma {sigma} b {b}: {cycles} cycles, {out['n_steps']} steps, worst inner {out['inner_worst']:.2e}")
    assert out["converged"] is True and cycles == EXACT_CYCLES[(sigma, b)]
    call = lambda name, *ints: (name, ints, None, False)
    check = r * [call("spmm", n, n), call("panel_gram", vs, r, n)] + r * [call("panel_apply", vs, r, n),
                                                                            call("spmm_resid", n, b)]
    want = [("block_lanczos_reorth", (m, LC, vs, PASSES), "inverse", False)]
    for c in range(1, cycles + 1):
        want += [compress(vs, m, r, n)] + check
        if c < cycles:
            want += [("block_lanczos_reorth_resume", (r, m, LC, vs, PASSES), "inverse", False)]
    want += [compress(vs, r, nch, n)]
    assert h.trace == want
    inv0, w0, _ = h.ops[0]
    assert all(i is inv0 and w is w0 for i, w, _ in h.ops) and w0.numel() == 5 * n * b
    steps = m + (cycles - 1) * (m - r)
    assert out["n_steps"] == out["inner_solves"] == out["inner_passes"] == steps and len(out["history"]) == cycles
    assert out["n_spmm"] == 3 * steps + 2 * r * cycles
    assert out["inner_not_met"] == 0 and out["inner_breakdown"] == 0 and out["inner_worst"] <= 1e-10
    assert out["sigma"] == sigma and out["inner"] == "minres"
    assert out["inner_tol"] == max(lz_factor(standin) * 1e-10, 64 * EPS)
    assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale",
                        "sigma", "inner", "inner_tol", "inner_solves", "inner_passes", "inner_not_met",
                        "inner_worst", "inner_breakdown", "n_steps"}


def lz_factor(standin):
    import sys
    return sys.modules["lanczos_amd"].INNER_TOL_FACTOR


def nearest(ev, sigma, nev):
    return ev[np.argsort(np.abs(ev - sigma), kind="stable")[:nev]]


@pytest.mark.parametrize("b", [4, 16])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_result(standin, solved, sigma, b):
    _, A, ev = standin
    h, out = solved[(sigma, b)]
    nev, scale = NEV[b], out["scale"]
    assert scale == 8.0  # gershgorin of the 5-point Laplacian
    theta, resid = out["theta"], out["resid"]
    # pair by pair: sorted by value, since two eigenvalues at nearly the same distance on either
    # side of sigma may change places in the distance order
    want = nearest(ev, sigma, nev)
    err = np.abs(np.sort(theta) - np.sort(want))
    bound = np.maximum(resid[np.argsort(theta)], 64 * EPS * scale)
    print(f"sigma {sigma} b {b}: max|theta - exact| {err.max():.3e}, resid {resid.max():.3e}")
    assert (err <= bound).all()
    assert (resid <= 1e-10 * scale).all()
    assert (np.diff(np.abs(theta - sigma)) >= 0).all(), "ordered by |lambda - sigma| ascending"
    nch = -(-nev // b)
    X = out["V"].numpy()[:nch * out["vstride"]].reshape(nch, out["vstride"])[:, :A.n * b].reshape(nch, A.n, b) \
        .transpose(1, 0, 2).reshape(A.n, nch * b)
    true = np.linalg.norm(A.dense @ X[:, :nev] - X[:, :nev] * theta, axis=0)
    assert np.abs(true - resid).max() <= 1e3 * EPS * scale
    assert np.abs(X[:, :nev].T @ X[:, :nev] - np.eye(nev)).max() <= 1e-10


@pytest.mark.parametrize("sigma", SIGMAS)
def test_default_inner_tol_keeps_the_exact_cycle_count(standin, sigma):
    """Inner solves perturbed to exactly the default inner tolerance: the same cycles as exact
    solves, the same stop test met (DESIGN.md 27's table, the row of INNER_TOL_FACTOR)."""
    tol = 1e-10
    h, out = run(standin, sigma, 16, rel=lz_factor(standin) * tol)
    assert out["converged"] is True and out["cycles"] == EXACT_CYCLES[(sigma, 16)]
    assert (out["resid"] <= tol * out["scale"]).all()
    assert out["inner_worst"] <= out["inner_tol"] * (1 + 1e-3) and out["inner_worst"] >= 0.5 * out["inner_tol"]


def test_sigma_none_is_the_old_path(lz):
    """The existing cases through the extended stand-in and eigsh's new signature: the trace
    test_restart_driver records and asserts, and the same dict keys."""
    standin = make_inverse_standin(lz)
    for name in ("dense-largest", "dense-smallest"):
        h, A, out = run_eigsh(lz, name, standin)
        _, nev, _, m, r, _, _, _ = EIGSH[name]
        assert h.trace == plain_trace(out["cycles"], A.n, m, r, -(-nev // B_))
        h0, _, out0 = run_eigsh(lz, name)
        assert h.trace == h0.trace and np.array_equal(out["theta"], out0["theta"])
        assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale"}


def test_cycle_cap_and_unmet_inner_solves(standin):
    """Inner solves a thousand times worse than the stop test allows: no exception, the cap."""
    h, out = run(standin, 0.5, 4, rel=1e-4, max_cycles=3)
    assert out["converged"] is False and out["cycles"] == 3 and len(out["history"]) == 3
    assert out["inner_not_met"] > 0 and out["inner_worst"] > out["inner_tol"]


def test_argument_errors(lz, standin):
    Handle, A, _ = standin
    h = Handle()
    for kw, text in [
        (dict(sigma=0.5, which="smallest"), "eigsh: sigma= selects the pairs nearest sigma; which must stay at its default"),
        (dict(sigma=0.5, filter_degree=8), "eigsh: sigma= and filter_degree= / cut= are mutually exclusive"),
        (dict(sigma=0.5, inner="gmres"), 'eigsh: inner is "minres", "columns" or "block"'),
        (dict(sigma=float("nan")), "eigsh: sigma must be finite"),
        (dict(sigma=0.5, inner_tol=0.0), "eigsh: inner_tol > 0"),
        (dict(sigma=0.5, m=4, keep=1), "eigsh: keep * b = 4 < nev = 6"),
    ]:
        with pytest.raises(lz.LanczosError) as e:
            h.eigsh(A, 6, b=B_, **kw)
        assert str(e.value) == text
    assert h.trace == []
    T, bm = np.eye(8), np.eye(2)
    with pytest.raises(ValueError):
        lz.ritz_pairs_dense(4, 2, T, bm, 3, "middle")
    with pytest.raises(ValueError):
        lz.restart_coeffs(4, 2, 1, T, bm, "middle")
    with pytest.raises(lz.LanczosError) as e:
        lz.Handle._reorth_op(h, "block_lanczos_reorth", A, A.n, 4, A.val, (8, 0.0, 1.0, 2.0), None, None, None,
                             (0.5, "minres", 1e-8, None, lz.InverseInfo()))
    assert "inverse= is mutually exclusive" in str(e.value)


def inner_tol_table(lz, tol=1e-10, b=16):
    """c -> per sigma (cycles, the largest wanted residual / scale at the end, converged)."""
    standin_ = make_inverse_standin(lz)
    Handle, Csr = standin_
    A = laplace(lz, Csr)
    st = (Handle, A, None)
    rows = {}
    for c in (0.0, 1e2, 1e1, 1.0, 1e-1, 1e-2, 1e-3):
        rows[c] = []
        for s in SIGMAS:
            h, out = run(st, s, b, rel=c * tol, tol=tol, max_cycles=12)
            rows[c].append((out["cycles"], out["history"][-1] / out["scale"], out["converged"]))
    return rows


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    for b in (16, 4):
        print(f"b = {b}: c, then (cycles, resid / scale, converged) at sigma = {SIGMAS}")
        for c, row in inner_tol_table(ge.load_package(), b=b).items():
            print(f"  {c:7.0e}  " + "  ".join(f"({cy}, {rs:.1e}, {cv})" for cy, rs, cv in row))
