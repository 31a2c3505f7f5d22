"""The thick-restart driver behind Handle.eigsh, its filtered form and Handle.svds, without a
GPU: a Handle whose device methods are dense fp64 NumPy restatements of their docstrings
runs the three solvers unchanged on CPU tensors and records every device call.

Checked per case: the sequence of device calls (written out here from the cycle count the
solve reports), the counters, the result against numpy.linalg on the dense matrix, the
filtered solve's early return, the cycle cap and the m / keep argument errors.
"""
import numpy as np
import pytest

B_, LC, PASSES = 4, 5, 2  # every case: b = 4, lc = 5, two reorthogonalisation passes


def make_standin(lz):
    """(DenseHandle, DenseCsr) for the package module lz."""
    import torch

    def np_(t):
        return t.numpy()  # CPU tensors: the array shares the tensor's memory

    class DenseCsr(lz.CsrDevice):
        """CPU tensors plus a dense fp64 copy."""

        def __init__(self, n, n_cols, row_ptr, col, val):
            super().__init__(n, n_cols, torch.from_numpy(np.ascontiguousarray(row_ptr, np.int64)),
                             torch.from_numpy(np.ascontiguousarray(col, np.int32)),
                             torch.from_numpy(np.ascontiguousarray(val, np.float64)))
            self.dense = np.zeros((n, n_cols))
            for row in range(n):
                s = slice(row_ptr[row], row_ptr[row + 1])
                self.dense[row, col[s]] = val[s]

        @classmethod
        def from_dense(cls, D):
            nz = D != 0
            rp = np.zeros(D.shape[0] + 1, np.int64)
            np.cumsum(nz.sum(axis=1), out=rp[1:])
            return cls(D.shape[0], D.shape[1], rp, np.nonzero(nz)[1], D[nz])

        def transpose(self, handle):
            return DenseCsr.from_dense(np.ascontiguousarray(self.dense.T))

    def sqrtm_pair(G):
        """As the device: beta = U sqrt|w| U^T, beta^-1 = U / sqrt|w| U^T (1 / 0 = inf, no
        exception), and a Gram that is not finite gives NaN blocks."""
        if not np.isfinite(G).all():
            return np.full_like(G, np.nan), np.full_like(G, np.nan)
        w, U = np.linalg.eigh(0.5 * (G + G.T))
        w = np.abs(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (U * np.sqrt(w)) @ U.T, (U / np.sqrt(w)) @ U.T

    def operator(A, filt, normal):
        """Q -> A Q, p(A) Q (the three-term recurrence of cheb_apply) or Pt (P Q)."""
        if normal is not None:
            P, Pt, _ = normal
            return lambda Q: Pt.dense @ (P.dense @ Q)
        if filt is None:
            return lambda Q: A.dense @ Q
        degree, lo, hi, ref = filt
        e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
        s1 = e / (ref - c0)

        def p(X):
            prev, cur, sg = X, (s1 / e) * (A.dense @ X) - (c0 * s1 / e) * X, s1
            for _ in range(2, degree + 1):
                sn = 1.0 / (2.0 / s1 - sg)
                prev, cur = cur, (2.0 * sn / e) * (A.dense @ cur) - (2.0 * sn * c0 / e) * cur - (sg * sn) * prev
                sg = sn
            return cur
        return p

    class DenseHandle(lz.Handle):
        """No device: the methods the solvers call, in fp64 NumPy, each recorded in trace as
        (name, its integer arguments, filt, normal is not None); ops keeps the operator
        keywords of the two kept-basis solves as passed."""

        def __init__(self):
            self._h = None
            self.trace, self.ops = [], []

        def close(self):
            pass

        def _steps(self, mul, j0, m, lc, S, q, alpha, beta, V, vstride, W, passes):
            """lanczos_cycle of test_restart_host.py on the flat panel."""
            n, b = W.shape
            q, alpha, beta, V, W = np_(q), np_(alpha), np_(beta), np_(V), np_(W)
            Q = lambda j: V[j * vstride:j * vstride + n * b].reshape(n, b)
            R = W.copy()
            for j in range(j0, m):
                beta[j], bi = sqrtm_pair(R.T @ R)
                Q(j)[:] = R @ bi
                q[j * b:(j + 1) * b] = Q(j)[lc]
                R = mul(Q(j))
                if S is not None and j == j0:
                    R = R - np.concatenate([Q(i) for i in range(j0)], axis=1) @ S
                elif j:
                    R = R - Q(j - 1) @ beta[j]
                a = R.T @ Q(j)
                alpha[j] = 0.5 * (a + a.T)
                R = R - Q(j) @ alpha[j]
                P = np.concatenate([Q(i) for i in range(j + 1)], axis=1)
                for _ in range(passes):
                    R = R - P @ (P.T @ R)
            beta[m] = sqrtm_pair(R.T @ R)[0]
            W[:] = R

        def block_lanczos_reorth(self, A, B, m, lc, q, alpha, beta, V, vstride, W, passes=2, filt=None, work=None,
                                 normal=None):
            self.trace.append(("block_lanczos_reorth", (m, lc, vstride, passes), filt, normal is not None))
            self.ops.append((filt, work, normal))
            W.copy_(B)
            self._steps(operator(A, filt, normal), 0, m, lc, None, q, alpha, beta, V, vstride, W, passes)

        def block_lanczos_reorth_resume(self, A, r, m, lc, sigma, q, alpha, beta, V, vstride, W, passes=2, filt=None,
                                        work=None, normal=None):
            self.trace.append(("block_lanczos_reorth_resume", (r, m, lc, vstride, passes), filt, normal is not None))
            self.ops.append((filt, work, normal))
            b = W.shape[1]
            self._steps(operator(A, filt, normal), r, m, lc, np_(sigma).reshape(r * b, b), q, alpha, beta, V, vstride,
                        W, passes)

        def panel_compress(self, V, vstride, k, r, Z, n=None):
            b = Z.shape[2]
            n = vstride // b if n is None else n
            self.trace.append(("panel_compress", (vstride, k, r, n), None, False))
            Vh = np_(V)
            blocks = np.stack([Vh[j * vstride:j * vstride + n * b].reshape(n, b) for j in range(k)])
            Y = np.einsum("jri,cjid->crd", blocks, np_(Z))
            for c in range(r):
                Vh[c * vstride:c * vstride + n * b] = Y[c].ravel()
            return V

        def spmm(self, A, X, Y, layout=lz.LZ_ROW_MAJOR):
            self.trace.append(("spmm", (A.n, A.n_cols), None, False))
            np_(Y)[:] = A.dense @ np_(X)
            return Y

        def mm_tt(self, W, R):
            self.trace.append(("mm_tt", tuple(W.shape), None, False))
            np_(R)[:] = np_(W).T @ np_(W)
            return R

        def mm_tt2(self, W, Q, R):
            self.trace.append(("mm_tt2", tuple(W.shape), None, False))
            np_(R)[:] = 0.5 * (np_(W).T @ np_(Q) + np_(Q).T @ np_(W))
            return R

        def mm_ts(self, beta, alpha, Q, S, W):
            self.trace.append(("mm_ts", tuple(Q.shape), None, False))
            QS = alpha * (np_(Q) @ np_(S))
            np_(W)[:] = QS if beta == 0 else beta * np_(W) + QS
            return W

    return DenseHandle, DenseCsr


# ------------------------------------------------------------------ the cases
def dense_sym():
    """n = 300, uniform(-1, 1) symmetrised, 20 + 3i added to diagonal entry 7i, i < 6."""
    rng = np.random.default_rng(3)
    D = rng.uniform(-1, 1, (300, 300))
    D = 0.5 * (D + D.T)
    for i in range(6):
        D[7 * i, 7 * i] += 20 + 3 * i
    return D


def rect(rows, cols):
    """uniform(-1, 1) at density 0.2 with 8 + 2i planted at (3 + 5i, 2 + 4i), i < 6."""
    rng = np.random.default_rng(9)
    D = rng.uniform(-1, 1, (rows, cols)) * (rng.uniform(0, 1, (rows, cols)) < 0.2)
    for i in range(6):
        D[3 + 5 * i, 2 + 4 * i] = 8 + 2 * i
    return D


# name: (operator, nev, which, m, keep, tol, filter_degree, max_cycles >= twice the measured count)
EIGSH = {
    "dense-largest": ("dense", 6, "largest", 6, 2, 1e-10, None, 20),
    "dense-smallest": ("dense", 6, "smallest", 6, 2, 1e-10, None, 200),
    "laplace-cheb12": ("laplace", 6, "smallest", 6, 2, 1e-9, 12, 12),
}
SVDS = {"tall": (90, 60), "wide": (60, 90)}  # k = 6, m = 6, keep = 3, tol 1e-9
SVDS_ARGS = dict(k=6, b=B_, m=6, keep=3, tol=1e-9, lc=LC, passes=PASSES)


def make_operator(lz, Csr, kind):
    if kind == "laplace":
        A = lz.gen_laplace2d(24, 20)
        return Csr(A.n, A.n, A.row_ptr, A.col, A.val)
    return Csr.from_dense(dense_sym() if kind == "dense" else rect(*SVDS[kind]))


def run_eigsh(lz, name, standin=None, **over):
    """A fresh stand-in handle, the case's operator and eigsh's result."""
    Handle, Csr = standin or make_standin(lz)
    kind, nev, which, m, keep, tol, degree, cap = EIGSH[name]
    h, A = Handle(), make_operator(lz, Csr, kind)
    args = dict(which=which, b=B_, m=m, keep=keep, tol=tol, max_cycles=cap, lc=LC, passes=PASSES,
                filter_degree=degree)
    args.update(over)
    return h, A, h.eigsh(A, nev, **args)


def run_svds(lz, name, standin=None, **over):
    Handle, Csr = standin or make_standin(lz)
    h, A = Handle(), make_operator(lz, Csr, name)
    return h, A, h.svds(A, **{**SVDS_ARGS, "max_cycles": 10, **over})


@pytest.fixture(scope="module")
def solved(lz):
    """Every case solved once; the tests below only read."""
    standin = make_standin(lz)
    out = {name: run_eigsh(lz, name, standin) for name in EIGSH}
    out.update({name: run_svds(lz, name, standin) for name in SVDS})
    return out


# ---------------------------------------------------------------- the traces
def first(m, vs, filt=None, normal=False):
    return ("block_lanczos_reorth", (m, LC, vs, PASSES), filt, normal)


def resume(r, m, vs, filt=None, normal=False):
    return ("block_lanczos_reorth_resume", (r, m, LC, vs, PASSES), filt, normal)


def compress(vs, k, r, n):
    return ("panel_compress", (vs, k, r, n), None, False)


def call(name, *ints):
    return (name, ints, None, False)


def plain_trace(cycles, n, m, r, nch, normal=False):
    """first(m), then (compress(m, r), resume(r, m)) for each cycle after the first, then compress(m, nch)."""
    vs = n * B_  # n * b is even at every case: the 16-byte stride adds nothing in fp64
    return ([first(m, vs, normal=normal)] + (cycles - 1) * [compress(vs, m, r, n), resume(r, m, vs, normal=normal)]
            + [compress(vs, m, nch, n)])


def same_operator(h, filt=False, normal=False):
    """One operator for every kept-basis call of a solve: the same filt value, the same work /
    normal objects (the filtered solve's first call is the unfiltered one)."""
    ops = h.ops[1:] if filt else h.ops
    f0, w0, n0 = ops[0]
    assert (f0 is not None) == filt and (n0 is not None) == normal and (w0 is not None) == filt
    for f, w, nm in ops:
        assert f == f0 and w is w0 and nm is n0
    if filt:
        assert h.ops[0] == (None, None, None)


@pytest.mark.parametrize("name", ["dense-largest", "dense-smallest"])
def test_eigsh_trace_and_counters(solved, name):
    h, A, out = solved[name]
    _, nev, _, m, r, _, _, cap = EIGSH[name]
    cycles, nch = out["cycles"], -(-nev // B_)
    print(f"{name}: {cycles} cycles, {out['n_spmm']} SpMMs")
    assert out["converged"] is True and cycles <= cap
    assert h.trace == plain_trace(cycles, A.n, m, r, nch)
    same_operator(h)
    assert out["n_spmm"] == m + (cycles - 1) * (m - r) and len(out["history"]) == cycles
    assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale"}


def test_eigsh_cheb_trace_and_counters(solved):
    h, A, out = solved["laplace-cheb12"]
    _, nev, _, m, r, _, degree, cap = EIGSH["laplace-cheb12"]
    n, cycles, nch = A.n, out["cycles"], -(-nev // B_)
    vs, filt = n * B_, out["filter"]
    print(f"laplace-cheb12: {cycles} filtered cycles, {out['n_steps']} steps, {out['n_spmm']} SpMMs")
    assert out["converged"] is True and 1 <= cycles <= cap
    assert filt[0] == degree and all(isinstance(x, float) for x in filt[1:])
    check = nch * [call("spmm", n, n), call("mm_tt2", n, B_), call("mm_ts", n, B_), call("mm_tt", n, B_)]
    want = [first(m, vs), first(m, vs, filt)]
    for c in range(1, cycles + 1):
        want += [compress(vs, m, r, n)] + check + ([resume(r, m, vs, filt)] if c < cycles else [])
    want += [compress(vs, nch, nch, n)]
    assert h.trace == want
    same_operator(h, filt=True)
    steps = 2 * m + (cycles - 1) * (m - r)
    assert out["n_steps"] == steps and len(out["history"]) == cycles
    assert out["n_spmm"] == m + (steps - m) * degree + cycles * nch


@pytest.mark.parametrize("name", list(SVDS))
def test_svds_trace_and_counters(solved, name):
    h, A, out = solved[name]
    k, m, r = SVDS_ARGS["k"], SVDS_ARGS["m"], SVDS_ARGS["keep"]
    n, p = min(SVDS[name]), max(SVDS[name])
    cycles, nch = out["cycles"], -(-k // B_)
    print(f"svds {name}: {cycles} cycles, {out['n_spmm']} SpMMs")
    assert out["converged"] is True and cycles <= 10
    finish = nch * [call("spmm", p, n), call("mm_tt", p, B_), call("mm_ts", p, B_), call("spmm", n, p),
                    call("mm_ts", n, B_), call("mm_tt", n, B_)]
    assert h.trace == plain_trace(cycles, n, m, r, nch, normal=True) + finish
    same_operator(h, normal=True)
    assert out["n_spmm"] == 2 * (m + (cycles - 1) * (m - r)) + 2 * nch and len(out["history"]) == cycles


# --------------------------------------------------------------- the results
def columns(V, vstride, rows, nblocks):
    """The (rows, nblocks * b) matrix of a block-major panel."""
    return V.numpy()[:nblocks * vstride].reshape(nblocks, vstride)[:, :rows * B_].reshape(nblocks, rows, B_) \
        .transpose(1, 0, 2).reshape(rows, nblocks * B_)


@pytest.mark.parametrize("name", list(EIGSH))
def test_eigsh_result(solved, name):
    """A Ritz value lies within its residual norm of an eigenvalue, and the stop test bounds
    that residual (the estimate, or the measured one of the filtered solve) by tol * scale:
    |theta - exact| <= tol * scale.  The residual recomputed from the returned panel gets a
    factor 10 for the gap between the estimate and the true norm."""
    h, A, out = solved[name]
    _, nev, which, m, r, tol, degree, _ = EIGSH[name]
    ev = np.linalg.eigvalsh(A.dense)
    exact = ev[:nev] if which == "smallest" else ev[::-1][:nev]
    nch = -(-nev // B_)
    Xp = columns(out["V"], out["vstride"], A.n, nch)
    X = Xp[:, out["cols"]] if degree else Xp[:, :nev]
    if not degree:
        assert (Xp[:, nev:] == 0).all(), "the last block is zero-padded"
    err = np.abs(out["theta"] - exact).max()
    true = np.linalg.norm(A.dense @ X - X * out["theta"], axis=0)
    print(f"{name}: max|theta - exact| {err:.3e}, recomputed residual {true.max():.3e}, reported "
          f"{out['resid'].max():.3e}, gap {np.abs(true - out['resid']).max():.3e} "
          f"(tol * scale {tol * out['scale']:.3e})")
    assert err <= tol * out["scale"]
    assert true.max() <= 10 * tol * out["scale"]
    assert np.abs(X.T @ X - np.eye(nev)).max() <= 1e-10


@pytest.mark.parametrize("name", list(SVDS))
def test_svds_result(solved, name):
    """The same argument on G = P^T P: theta_i = s_i^2 lies within est_i of an eigenvalue of G,
    and the stop test gives est_i <= tol * s_max * max(s_i, sqrt(eps) s_max), so that
    |s_i - exact_i| = |theta_i - exact_i^2| / (s_i + exact_i) <= est_i / s_i
    <= tol * s_max / max(s_i, sqrt(eps) s_max) * s_max."""
    h, A, out = solved[name]
    k, tol = SVDS_ARGS["k"], SVDS_ARGS["tol"]
    R, C = SVDS[name]
    sv = np.linalg.svd(A.dense, compute_uv=False)
    s, smax = out["s"], sv[0]
    bound = tol * smax / np.maximum(s, np.sqrt(np.finfo(np.float64).eps) * smax) * smax
    nch = -(-k // B_)
    U = columns(out["U"], out["ustride"], R, nch)[:, :k]
    V = columns(out["V"], out["vstride"], C, nch)[:, :k]
    left = np.linalg.norm(A.dense.T @ U - V * s, axis=0)
    right = np.linalg.norm(A.dense @ V - U * s, axis=0)
    print(f"svds {name}: max|s - exact| {np.abs(s - sv[:k]).max():.3e}, residuals {max(left.max(), right.max()):.3e}, "
          f"reported {out['resid'].max():.3e} (tol * s_max {tol * smax:.3e})")
    assert (np.abs(s - sv[:k]) <= bound).all()
    assert max(left.max(), right.max()) <= 10 * tol * smax and out["resid"].max() <= 10 * tol * smax
    assert (np.diff(s) <= 0).all() and out["At"].dense.shape == (C, R)


# ------------------------------------------------- early return, cap, errors
def test_cheb_early_return(lz):
    """m = 24 blocks resolve the six planted eigenvalues to 2e-10 * scale in the unfiltered solve
    (1.5e-6 at m = 16): at tol 1e-6 the filtered solve returns there, as the unfiltered eigsh would."""
    h, A, out = run_eigsh(lz, "dense-largest", m=24, tol=1e-6, filter_degree=8)
    n, nev, nch = A.n, 6, 2
    assert out["cycles"] == 0 and out["filter"] is None and np.array_equal(out["cols"], np.arange(nev))
    assert out["converged"] is True and out["n_spmm"] == out["n_steps"] == 24 and len(out["history"]) == 1
    assert h.trace == [first(24, n * B_), compress(n * B_, 24, nch, n)]
    ev = np.linalg.eigvalsh(A.dense)[::-1][:nev]
    assert np.abs(out["theta"] - ev).max() <= 1e-6 * out["scale"]


@pytest.mark.parametrize("name", ["dense-largest", "laplace-cheb12", "tall"])
def test_cycle_cap(lz, name):
    h, A, out = (run_svds if name in SVDS else run_eigsh)(lz, name, max_cycles=2)
    assert out["converged"] is False and out["cycles"] == 2 and len(out["history"]) == 2


@pytest.mark.parametrize("who,count", [("eigsh", "nev"), ("svds", "k")])
def test_argument_errors(lz, who, count):
    Handle, Csr = make_standin(lz)
    h, A = Handle(), make_operator(lz, Csr, "tall")
    solve = getattr(h, who)
    for args, text in [
        (dict(m=4, keep=1), f"{who}: keep * b = 4 < {count} = 6"),
        (dict(m=2, keep=2), f"{who}: keep = 2 >= m = 2"),
        (dict(m=20, keep=17), f"{who}: 1 <= keep <= 16 and m <= 64"),
        (dict(m=65, keep=2), f"{who}: 1 <= keep <= 16 and m <= 64"),
    ]:
        with pytest.raises(lz.LanczosError) as e:
            solve(A, 6, b=B_, **args)
        assert str(e.value) == text
    assert h.trace == []
