"""Batched MINRES on the device: lz_minres_update (both forms of k_minres_update) and
Handle.solve(method="minres") (lz_minres_solve).

minres_update: each of u', d', X elementwise against the fp64 evaluation of the documented order,
within 3 eps(dtype) x (the sum of the absolute values of that expression's terms), the error of d'
carried into X's bound; uu against the device's own u' with test_gpu_kpm's reduction bound.
solve: test_gpu_cg.check_solve's checks -- the NumPy fp64 residual of the returned X, the returned
resid, est, the iteration counts and the SpMM count -- against test_minres_host's restatement.
"""
import itertools
import math

import numpy as np
import pytest

import test_gpu_cg
from test_cg_host import MET, SPENT, dense
from test_gpu_cg import EPS, EPS64, F32, F64, FORM128, GENERIC, TOL, check_solve, dev, f64, rhs, update_rows
from test_minres_host import BREAKDOWN, minres_operator, minres_restated

pytestmark = pytest.mark.gpu

NAMES = "W U Uo D1 D2 X".split()
A_W, A_U, A_O, G_O, G_1, G_2, TAU = range(7)


# ------------------------------------------------------------ 1. minres_update
def update_inputs(n, b, dtype, seed):
    """Six uniform(-1, 1) blocks and 7 b uniform(-2, 2) coefficients with a frozen column (seven
    zeros), a first-pass column (a_o = g_o = g_1 = g_2 = tau = 0; its Uo, D1, D2 NaN) and a
    second-pass column (g_2 = 0, its D2 NaN).  b = 1: the kind of its one column by seed % 4."""
    rng = np.random.default_rng(seed)
    blk = {k: rng.uniform(-1, 1, (n, b)).astype(dtype) for k in NAMES}
    coef = rng.uniform(-2, 2, (7, b))
    if b > 2:
        zc, fc, sc = b // 2, (b // 2 + 1) % b, (b // 2 + 2) % b
    else:
        zc, fc, sc = [(None, None, None), (0, None, None), (None, 0, None), (None, None, 0)][seed % 4]
    if zc is not None:
        coef[:, zc] = 0.0
    if fc is not None:
        coef[[A_O, G_O, G_1, G_2, TAU], fc] = 0.0
        for k in ("Uo", "D1", "D2"):
            blk[k][:, fc] = np.nan
    if sc is not None:
        coef[G_2, sc] = 0.0
        blk["D2"][:, sc] = np.nan
    return blk, coef, zc


def run_update(handle, torch, n, b, dtype, seed):
    blk, coef, zc = update_inputs(n, b, dtype, seed)
    d = {k: dev(torch, a) for k, a in blk.items()}
    cf = dev(torch, coef.reshape(-1))
    uu = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    handle.minres_update(cf, *(d[k] for k in NAMES), uu=uu)
    return blk, coef, zc, d, cf, uu


def check_update(lz, handle, torch, n, b, dtype, seed=0):
    blk, coef, zc, d, cf, uu = run_update(handle, torch, n, b, dtype, seed)
    eps, what = EPS[dtype], f"n={n} b={b} {dtype.__name__}"
    c = f64(coef.astype(dtype))
    term = lambda k, name: np.where(c[k] == 0, 0.0, c[k] * np.where(c[k] == 0, 0.0, f64(blk[name])))
    tu = [term(A_W, "W"), term(A_U, "U"), term(A_O, "Uo")]
    td = [term(G_O, "Uo"), term(G_1, "D1"), term(G_2, "D2")]
    u1, d1, x = sum(tu), sum(td), f64(blk["X"])
    x1 = c[TAU] * d1 + x
    dU = 3 * eps * sum(np.abs(t) for t in tu)
    dD = 3 * eps * sum(np.abs(t) for t in td)
    dX = 3 * eps * (np.abs(c[TAU] * d1) + np.abs(x)) + np.abs(c[TAU]) * dD
    got = {"u'": f64(d["Uo"].cpu().numpy()), "d'": f64(d["D2"].cpu().numpy()), "X": f64(d["X"].cpu().numpy())}
    worst = 0.0
    for k, ref, bound in (("u'", u1, dU), ("d'", d1, dD), ("X", x1, dX)):
        assert np.isfinite(got[k]).all(), f"{what}: NaN / Inf in {k}"
        err = np.abs(got[k] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"{what}: {k}"
    for k in ("W", "U", "D1"):
        assert np.array_equal(d[k].cpu().numpy().view(np.uint8), blk[k].view(np.uint8)), f"{what}: {k} is read only"
    assert torch.equal(cf, dev(torch, coef.reshape(-1))), f"{what}: coef is read only"
    if zc is not None:
        assert torch.equal(d["X"][:, zc], dev(torch, blk["X"][:, zc])), f"{what}: seven zeros leave X bit for bit"
        assert (d["Uo"][:, zc] == 0).all() and (d["D2"][:, zc] == 0).all(), f"{what}: a frozen column stores zeros"
    uuh, sq = uu.cpu().numpy(), (got["u'"] ** 2).sum(axis=0)
    assert np.isfinite(uuh).all(), f"{what}: NaN in uu"
    rerr = np.abs(uuh - sq)
    print(f"{what}: max err/bound {worst:.3f}; uu max err/bound "
          f"{(rerr / np.maximum((n + 2) * EPS64 * sq, 1e-300)).max():.3e}")
    assert (rerr <= (n + 2) * EPS64 * sq).all(), f"{what}: uu"
    return d["Uo"], d["D2"], d["X"], uu


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_update_parity(lz, handle, torch_cuda, b, dtype):
    rpb, rows = update_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) > lz.CG_GRID_CAP and math.ceil(rows[-2] / rpb) == 257
    for n in rows:
        check_update(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
    if b == 1:  # every kind of its one column
        for seed in range(4):
            check_update(lz, handle, torch_cuda, rows[3], b, dtype, seed=seed)


@pytest.mark.parametrize("b,dtype", FORM128)
def test_update_forms_agree(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """The 128-byte-row form and the generic form finish every element with the same operations:
    the same bits in u', d', X (uu sums in another order: each within its bound, above); two runs
    of a form give the same bits, uu included; plain loads and stores change no bit."""
    eq = torch_cuda.equal
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        fast = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        fast2 = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_GENERIC", "1")
            gen = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
            gen2 = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for k, u, v in zip(("u'", "d'", "X"), fast[:3], gen[:3]):
            assert eq(u, v), f"n={n}: {k} differs between the forms"
        for u, v in zip(fast + gen, fast2 + gen2):
            assert eq(u, v), f"n={n}: two runs differ"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_NT", "0")
            plain = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for u, v in zip(fast, plain):
            assert eq(u, v), "plain loads and stores: every bit, uu included"


def test_update_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    blocks = [torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(6)]
    cf = torch.zeros(7 * b, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for i, j in itertools.combinations(range(6), 2):
        args = list(blocks)
        args[j] = args[i]
        with pytest.raises(E):
            handle.minres_update(cf, *args)
    assert b"argument error" in handle.L.lz_last_error()
    for bad in (cf[:2 * b], cf[:7 * b - 1], cf.float()):
        with pytest.raises(E):
            handle.minres_update(bad, *blocks)
    with pytest.raises(E):
        handle.minres_update(cf, *blocks[:5], blocks[5][:, :8])
    with pytest.raises(E):
        handle.minres_update(cf, *blocks[:5], blocks[5].float())
    with pytest.raises(E):
        handle.minres_update(cf, *blocks, uu=torch.zeros(b + 1, dtype=torch.float64, device="cuda"))
    big = [torch.zeros(n, 65, dtype=torch.float64, device="cuda") for _ in range(6)]
    with pytest.raises(E):
        handle.minres_update(torch.zeros(7 * 65, dtype=torch.float64, device="cuda"), *big)
    assert b"argument error" in handle.L.lz_last_error()
    handle.minres_update(cf, *blocks)  # the call after the errors succeeds


# ------------------------------------------------------------ 2. solve
def minres_case(lz, handle, torch, name, b, dtype, **kw):
    """check_solve on method="minres", its yardstick the MINRES restatement (placed in
    test_gpu_cg's cache of restatements under this case's key); then the restarts."""
    A, shift, _ = minres_operator(lz, name, dtype)
    key = f"minres {name} b={b} {dtype.__name__}"
    if key not in test_gpu_cg.REF:
        test_gpu_cg.REF[key] = minres_restated(lz, A, rhs(A.n, b, dtype), shift=shift, tol=TOL[dtype], dtype=dtype)
    ref = test_gpu_cg.REF[key]
    assert (ref["status"] == MET).all()
    out, Bh, S, kernel = check_solve(lz, handle, torch, key, A, b, dtype, shift=shift, method="minres", **kw)
    assert out["method"] == "minres" and out["restarts"] <= ref["restarts"] + 1
    return A, shift, out, kernel


SADDLES = ["saddle47", "saddle48", "saddle49", "saddle1000", "saddle4099", "saddle20011", "saddlewide"]


@pytest.mark.parametrize("name", SADDLES)
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_saddle(lz, handle, torch_cuda, b, dtype, name):
    """[[S1, E], [E^T, -S2]]: as many negative as positive eigenvalues, |lambda| >= 1.  128-byte rows:
    the SpMM under the solve is the fused one, its dots leaving the store."""
    A, shift, out, kernel = minres_case(lz, handle, torch_cuda, name, b, dtype)
    assert kernel & lz.LZ_K_DOT, f"kernel id {kernel:#x}"
    if A.n <= 1000 and dtype == F64:
        lam = np.linalg.eigvalsh(dense(A) + shift * np.eye(A.n))
        assert int((lam < 0).sum()) == A.n - A.n // 2 and int((lam > 0).sum()) == A.n // 2
        assert np.abs(lam).min() >= 1 - 1e-12


@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype):
    """A negative 1 x 1 operator: u_2 = 0 up to rounding, one step."""
    A, shift, out, _ = minres_case(lz, handle, torch_cuda, "saddle1", b, dtype)
    assert A.n == 1 and float(A.val[0]) + shift < 0 and out["iters"].max() == 1


@pytest.mark.parametrize("b,dtype", GENERIC)
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype):
    *_, kernel = minres_case(lz, handle, torch_cuda, "saddle1000", b, dtype)
    assert not kernel & lz.LZ_K_DOT


@pytest.mark.parametrize("name,b,dtype", [("helm40x36", 16, F64), ("helm7x7", 16, F64), ("helm7x7", 32, F32)])
def test_solve_helmholtz(lz, handle, torch_cuda, name, b, dtype):
    """The 5-point Laplacian shifted into its spectrum: 55 negative eigenvalues, the nearest 3.5e-3
    from the shift (40 x 36, -0.5); 3 negative (7 x 7, -1)."""
    A, shift, out, _ = minres_case(lz, handle, torch_cuda, name, b, dtype)
    if dtype == F64:
        lam = np.linalg.eigvalsh(dense(A) + shift * np.eye(A.n))
        assert int((lam < 0).sum()) == minres_operator(lz, name, dtype)[2] and np.abs(lam).min() > 1e-3


def test_solve_spd(lz, handle, torch_cuda):
    """MINRES on a positive definite system behaves: the plain 40 x 36 Laplacian."""
    minres_case(lz, handle, torch_cuda, "lap40x36", 16, F64)


# ------------------------------------------------------------ 3. semantics
SHIFT = -0.5


@pytest.fixture(scope="module")
def helm(lz, handle, torch_cuda):
    """The 40 x 36 Laplacian at fp64 with shift -0.5, b = 16: the operator, its right-hand sides
    and one MINRES solve."""
    class P:
        pass
    s = P()
    s.A = lz.gen_laplace2d(40, 36)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.solve = lambda B=None, **kw: handle.solve(s.Ad, s.B if B is None else B, shift=SHIFT, method="minres", **kw)
    s.out = s.solve()
    assert s.out["converged"].all() and s.out["restarts"] == 0
    return s


def test_cg_does_not_reach_it(lz, helm, handle):
    o = handle.solve(helm.Ad, helm.B, shift=SHIFT)
    nz = np.arange(16) != 3
    assert (((o["status"] == BREAKDOWN) | ((o["status"] == SPENT) & (o["resid"] > 1e-10)))[nz]).all()
    assert (helm.out["resid"] <= 1e-10).all() and (helm.out["status"] == MET).all()


def test_zero_column(lz, helm, torch_cuda):
    o = helm.out
    assert o["iters"][3] == 0 and o["status"][3] == MET and o["resid"][3] == 0 and o["est"][3] == 0
    assert (o["X"][:, 3] == 0).all()
    assert torch_cuda.isfinite(o["X"]).all() and np.isfinite(o["resid"]).all() and np.isfinite(o["est"]).all()


def test_converged_start(lz, helm, torch_cuda):
    again = helm.solve(X0=helm.out["X"])
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], helm.out["X"])
    assert np.array_equal(again["resid"], helm.out["resid"])


@pytest.mark.parametrize("j", [5, 15])
def test_independent_columns(lz, helm, torch_cuda, j):
    B2h = np.repeat(helm.Bh[:, :1], 16, axis=1)
    B2h[:, j] = helm.Bh[:, j]
    o2 = helm.solve(dev(torch_cuda, B2h))
    assert o2["restarts"] == 0
    assert torch_cuda.equal(o2["X"][:, j], helm.out["X"][:, j]) and o2["iters"][j] == helm.out["iters"][j]
    assert o2["resid"][j] == helm.out["resid"][j] and o2["est"][j] == helm.out["est"][j]


def test_reproducible(lz, helm, torch_cuda):
    again = helm.solve()
    assert torch_cuda.equal(again["X"], helm.out["X"]) and np.array_equal(again["iters"], helm.out["iters"])
    assert np.array_equal(again["resid"], helm.out["resid"]) and np.array_equal(again["est"], helm.out["est"])


def test_check_every(lz, helm, torch_cuda):
    o1, o8, o16 = (helm.solve(check_every=k) for k in (1, 8, 16))
    for o in (o1, o8, o16):
        assert torch_cuda.equal(o["X"], helm.out["X"]) and np.array_equal(o["iters"], helm.out["iters"])
    # a column that takes k steps runs k + 1 passes
    assert o1["iterations"] == o1["iters"].max() + 1
    assert o1["iterations"] <= o8["iterations"] < o1["iterations"] + 8
    assert o1["iterations"] <= o16["iterations"] < o1["iterations"] + 16
    assert o8["iterations"] % 8 == 0 and o16["iterations"] % 16 == 0


def test_max_iter(lz, helm, torch_cuda):
    o = helm.solve(max_iter=5)
    nz = np.arange(16) != 3
    assert (o["status"][nz] == SPENT).all() and (o["iters"][nz] == 5).all() and o["iters"][3] == 0
    assert o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()
    assert o["n_spmm"] == o["iterations"] + 2 and o["iterations"] == 8  # 6 passes, enqueued in chunks of 8
    o0 = helm.solve(max_iter=0)
    assert (o0["status"][nz] == SPENT).all() and (o0["iters"] == 0).all() and o0["n_spmm"] == 1


def test_nan_column(lz, helm, torch_cuda):
    B2h = helm.Bh.copy()
    B2h[7, 9] = np.nan
    X0 = dev(torch_cuda, np.random.default_rng(1).uniform(-1, 1, helm.Bh.shape))
    X0[:, 3] = 0  # (the zero column: with any other start nothing meets tol |b| = 0)
    keep = X0.clone()
    o = helm.solve(dev(torch_cuda, B2h), X0=X0)
    clean = helm.solve(X0=X0)
    ok = np.arange(16) != 9
    assert o["status"][9] == BREAKDOWN and o["iters"][9] == 0 and not o["converged"][9]
    assert torch_cuda.equal(o["X"][:, 9], keep[:, 9]) and torch_cuda.equal(X0, keep)
    assert (o["status"][ok] == MET).all() and (clean["status"] == MET).all()
    assert torch_cuda.equal(o["X"][:, ok], clean["X"][:, ok]) and np.array_equal(o["iters"][ok], clean["iters"][ok])


def test_arguments(lz, helm, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = helm.A.n, 16
    with pytest.raises(E, match="preconditioner"):
        helm.solve(precond="jacobi")
    with pytest.raises(E, match='"columns", "block" or "minres"'):
        handle.solve(helm.Ad, helm.B, method="gmres")
    buf = torch.zeros(7 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        helm.solve(work=buf[:4 * n * b])                               # work too short (5 blocks)
    with pytest.raises(E):                                             # work holds B
        helm.solve(buf[n * b:2 * n * b].view(n, b), work=buf[:5 * n * b])
    with pytest.raises(E):
        helm.solve(torch.zeros(n, 65, dtype=torch.float64, device="cuda"))
    with pytest.raises(E):
        helm.solve(tol=0.0)
    assert b"argument error" in handle.L.lz_last_error()
    o = helm.solve(work=buf[:5 * n * b])                               # the call after the errors succeeds
    assert torch.equal(o["X"], helm.out["X"])
    assert torch.equal(helm.B, dev(torch, helm.Bh)), "B is read only"


# ------------------------------------------------------------ 4. history
@pytest.mark.parametrize("poison", ["1", "0"])
def test_history(lz, helm, torch_cuda, monkeypatch, poison):
    """A column solve, a Jacobi solve, a block solve and a spectral_moments call share cg_ws and
    dots_ws with the MINRES solve that follows them on one handle: it gives the bits of the same
    solve on a handle of its own, with the workspaces NaN-filled at creation and growth or not
    (LZ_POISON is read by lz_init and by the growers)."""
    monkeypatch.setenv("LZ_POISON", poison)
    used, fresh = lz.Handle(0), lz.Handle(0)
    try:
        spd = dict(shift=1.0)
        used.solve(helm.Ad, helm.B, **spd)
        used.solve(helm.Ad, helm.B, precond="jacobi", **spd)
        used.solve(helm.Ad, helm.B, method="block", **spd)
        used.spectral_moments(helm.Ad, n_moments=19, b=16, seed=3)
        outs = [h.solve(helm.Ad, helm.B, shift=SHIFT, method="minres") for h in (used, fresh)]
        torch_cuda.cuda.synchronize()
        assert used.device_error() == 0 and fresh.device_error() == 0
    finally:
        used.close()
        fresh.close()
    for o in outs:
        assert torch_cuda.equal(o["X"], helm.out["X"]) and np.array_equal(o["iters"], helm.out["iters"])
        assert np.array_equal(o["resid"], helm.out["resid"]) and np.array_equal(o["est"], helm.out["est"])
        assert o["n_spmm"] == helm.out["n_spmm"] and np.array_equal(o["status"], helm.out["status"])
