"""Block conjugate gradients on the device: lz_bcg_update, lz_bcg_direction (the b = 16 fp64
and b = 32 fp32 MFMA kernels and the generic ones) and Handle.solve(method="block") (lz_bcg_solve).

The two passes: each output element against the fp64 NumPy evaluation within (b + 2) eps(dtype)
x (the sum of the absolute values of its terms), the factors rounded to the blocks' dtype first
and the error of the new Q carried into S's bound; G against the device's own stored Q with
test_gpu_kpm's reduction bound.  The solves: the NumPy fp64 residual of the returned X, the
returned resid, and the iteration counts against test_bcg_host's restatement of the loop.
"""
import ctypes
import math

import numpy as np
import pytest

from test_bcg_host import (CONVERGED, MET, NOT_PD, R_NOT_PD, R_SPENT, RANK, SPENT, bcg_restated, bcg_rhs,
                           fallback_case, FALLBACKS)
from test_cg_host import gersh_shift, lap_B, sp_csr
from test_gpu_cheb import fused_operator

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
EPS64 = EPS[F64]
HOT = [(16, F64), (32, F32)]
GENERIC = [(1, F64), (5, F64), (8, F64), (16, F32)]
TOL = {F64: 1e-10, F32: 1e-4}


def f64(x):
    return np.asarray(x, F64)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------ 1. the two passes
RAN = {}   # the dense kernel id after the last update / direction call (lz_debug_last_kernel)


def pass_rows(lz, b, dtype, generic=False):
    """(tile, rows per block pass, the sizes): 1; a tile - 1, equal, + 1; a block pass - 1, equal,
    + 1; the grid cap's rows + 1 (the grid-stride loop's second trip)."""
    if (b, dtype) == (16, F64) and not generic:
        tile, rpb = 16, lz.BCG_ROWS_16
    elif (b, dtype) == (32, F32) and not generic:
        tile, rpb = 32, lz.BCG_ROWS_32
    else:
        tile, rpb = lz.BCG_ROWS_GEN, lz.BCG_ROWS_GEN
    rows = {1, tile - 1, tile, tile + 1, rpb - 1, rpb, rpb + 1, lz.BCG_GRID_CAP * rpb + 1}
    return tile, rpb, sorted(rows)


def kernel_id(lz, b, dtype, generic=False):
    """The id lz_debug_last_kernel reports for the two passes at this shape."""
    if generic:
        return lz.LZ_K_BCG_GEN
    return {(16, F64): lz.LZ_K_BCG16, (32, F32): lz.LZ_K_BCG32F}.get((b, dtype), lz.LZ_K_BCG_GEN)


def spd_factor(rng, b):
    M = rng.uniform(-1, 1, (2 * b + 1, b))
    return M.T @ M / b + 0.1 * np.eye(b)


def update_case(lz, handle, torch, n, b, dtype, seed):
    rng = np.random.default_rng(seed)
    Sh, Wh, Qh, Xh = (rng.uniform(-1, 1, (n, b)).astype(dtype) for _ in range(4))
    xi, E = spd_factor(rng, b), rng.uniform(-1, 1, (b, b))
    S, W, Q, X = (dev(torch, a) for a in (Sh, Wh, Qh, Xh))
    xid, Ed = dev(torch, xi), dev(torch, E)
    G = torch.full((b, b), float("nan"), dtype=torch.float64, device="cuda")
    handle.bcg_update(xid, Ed, S, W, Q, X, G=G)
    RAN["update"] = handle.last_kernel()[1]
    assert torch.equal(S, dev(torch, Sh)) and torch.equal(W, dev(torch, Wh)), "S and W are read only"
    assert torch.equal(xid, dev(torch, xi)) and torch.equal(Ed, dev(torch, E)), "xi and E are read only"
    eps = EPS[dtype]
    s, w, q, x = f64(Sh), f64(Wh), f64(Qh), f64(Xh)
    xr, er = f64(xi.astype(dtype)), f64(E.astype(dtype))
    refX, refQ = x + s @ er, q - w @ xr
    bX = (b + 2) * eps * (np.abs(x) + np.abs(s) @ np.abs(er))
    bQ = (b + 2) * eps * (np.abs(q) + np.abs(w) @ np.abs(xr))
    return (Q, X, G), (refQ, refX), (bQ, bX)


def check_update(lz, handle, torch, n, b, dtype, seed=0):
    (Q, X, G), (refQ, refX), (bQ, bX) = update_case(lz, handle, torch, n, b, dtype, seed)
    what = f"update n={n} b={b} {dtype.__name__}"
    Qd, Xd, Gd = f64(Q.cpu().numpy()), f64(X.cpu().numpy()), G.cpu().numpy()
    assert np.isfinite(Qd).all() and np.isfinite(Xd).all() and np.isfinite(Gd).all(), what
    eQ, eX = np.abs(Qd - refQ), np.abs(Xd - refX)
    ref = Qd.T @ Qd
    gb = (n + 2) * EPS64 * (np.abs(Qd).T @ np.abs(Qd))
    eG = np.abs(Gd - ref)
    print(f"{what}: max err/bound Q {(eQ / bQ).max():.3f}, X {(eX / bX).max():.3f}, G {(eG / gb).max():.3e}")
    assert (eQ <= bQ).all(), f"{what}: Q"
    assert (eX <= bX).all(), f"{what}: X"
    assert (eG <= gb).all(), f"{what}: G against the stored Q"
    return Qd, Xd, Gd, bQ, bX, gb


def check_direction(lz, handle, torch, n, b, dtype, seed=0):
    rng = np.random.default_rng(seed + 1)
    Qh, Sh = (rng.uniform(-1, 1, (n, b)).astype(dtype) for _ in range(2))
    z = spd_factor(rng, b)
    zi = np.linalg.inv(z)
    Q, S, zd, zid = dev(torch, Qh), dev(torch, Sh), dev(torch, z), dev(torch, zi)
    handle.bcg_direction(zd, zid, Q, S)
    RAN["direction"] = handle.last_kernel()[1]
    assert torch.equal(zd, dev(torch, z)) and torch.equal(zid, dev(torch, zi)), "z and zinv are read only"
    eps, what = EPS[dtype], f"direction n={n} b={b} {dtype.__name__}"
    q, s, zr, zir = f64(Qh), f64(Sh), f64(z.astype(dtype)), f64(zi.astype(dtype))
    refQ = q @ zir
    bQ = (b + 2) * eps * (np.abs(q) @ np.abs(zir))
    refS = refQ + s @ zr
    bS = (b + 2) * eps * (np.abs(refQ) + np.abs(s) @ np.abs(zr)) + bQ   # the new Q's error carried
    Qd, Sd = f64(Q.cpu().numpy()), f64(S.cpu().numpy())
    assert np.isfinite(Qd).all() and np.isfinite(Sd).all(), what
    eQ, eS = np.abs(Qd - refQ), np.abs(Sd - refS)
    print(f"{what}: max err/bound Q {(eQ / np.maximum(bQ, 1e-300)).max():.3f}, S {(eS / bS).max():.3f}")
    assert (eQ <= bQ).all(), f"{what}: Q"
    assert (eS <= bS).all(), f"{what}: S"
    return Qd, Sd, bQ, bS


@pytest.mark.parametrize("b,dtype", HOT + GENERIC)
def test_pass_parity(lz, handle, torch_cuda, b, dtype):
    tile, rpb, rows = pass_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) == lz.BCG_GRID_CAP + 1
    for n in rows:
        check_update(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
        check_direction(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
        assert RAN == {"update": kernel_id(lz, b, dtype), "direction": kernel_id(lz, b, dtype)}, f"n={n}: {RAN}"


@pytest.mark.parametrize("b,dtype", HOT)
def test_mfma_against_generic(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """Both hot shapes: the MFMA kernels against the generic ones (LZ_BCG_GENERIC=1) within the bound
    each is held to against NumPy; either store flavour forced (LZ_BCG_NT) gives the same bits."""
    _, _, rows = pass_rows(lz, b, dtype)
    _, _, gen_rows = pass_rows(lz, b, dtype, generic=True)
    for n in sorted({rows[0], rows[3], rows[6], rows[-1], gen_rows[-1]}):
        fast_u = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
        fast_d = check_direction(lz, handle, torch_cuda, n, b, dtype, seed=7)
        assert set(RAN.values()) == {kernel_id(lz, b, dtype)} != {lz.LZ_K_BCG_GEN}
        with monkeypatch.context() as mp:
            mp.setenv("LZ_BCG_GENERIC", "1")
            gen_u = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
            gen_d = check_direction(lz, handle, torch_cuda, n, b, dtype, seed=7)
            assert set(RAN.values()) == {lz.LZ_K_BCG_GEN}
        Qf, Xf, Gf, bQ, bX, gb = fast_u
        assert (np.abs(Qf - gen_u[0]) <= bQ).all() and (np.abs(Xf - gen_u[1]) <= bX).all()
        # (G is a function of each form's own Q: the reduction bound plus the Q difference's share)
        dG = np.abs(Qf - gen_u[0]).T @ np.abs(Qf) + np.abs(Qf).T @ np.abs(Qf - gen_u[0])
        assert (np.abs(Gf - gen_u[2]) <= 2 * gb + 1.01 * dG).all()
        assert (np.abs(fast_d[0] - gen_d[0]) <= fast_d[2]).all() and (np.abs(fast_d[1] - gen_d[1]) <= fast_d[3]).all()
        for flavour in ("0", "1"):      # plain and non-temporal streams forced: the shipped form's bits
            with monkeypatch.context() as mp:
                mp.setenv("LZ_BCG_NT", flavour)
                forced_u = check_update(lz, handle, torch_cuda, n, b, dtype, seed=7)
                forced_d = check_direction(lz, handle, torch_cuda, n, b, dtype, seed=7)
                assert set(RAN.values()) == {kernel_id(lz, b, dtype)}
            for u, v in zip(fast_u[:3] + fast_d[:2], forced_u[:3] + forced_d[:2]):
                assert np.array_equal(u, v), f"LZ_BCG_NT={flavour}: every bit"


def test_pass_reproducible(lz, handle, torch_cuda):
    for b, dtype in HOT:
        n = pass_rows(lz, b, dtype)[2][-1]
        a, c = (check_update(lz, handle, torch_cuda, n, b, dtype, seed=3) for _ in range(2))
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], c[:3])), "two runs, the same bits (G included)"


def test_misaligned_blocks_take_the_generic_kernels(lz, handle, torch_cuda):
    """Blocks off a 16-byte boundary (a view one fp64 element into a buffer): the generic kernels,
    reported as such, and the same values within the bound."""
    torch, n, b = torch_cuda, 100, 16
    rng = np.random.default_rng(4)
    hs = [rng.uniform(-1, 1, (n, b)) for _ in range(4)]
    xi, E = spd_factor(rng, b), rng.uniform(-1, 1, (b, b))
    outs = []
    for off in (0, 1):
        blocks = []
        for a in hs:
            buf = torch.zeros(n * b + 2, dtype=torch.float64, device="cuda")
            v = buf[off:off + n * b].view(n, b)
            v.copy_(dev(torch, a))
            blocks.append(v)
        S, W, Q, X = blocks
        G = handle.bcg_update(dev(torch, xi), dev(torch, E), S, W, Q, X)
        assert handle.last_kernel()[1] == (lz.LZ_K_BCG_GEN if off else lz.LZ_K_BCG16)
        outs.append((f64(Q.cpu().numpy()), f64(X.cpu().numpy()), G.cpu().numpy()))
    s, w, q, x = hs
    bQ = (b + 2) * EPS64 * (np.abs(q) + np.abs(w) @ np.abs(xi))
    bX = (b + 2) * EPS64 * (np.abs(x) + np.abs(s) @ np.abs(E))
    assert (np.abs(outs[0][0] - outs[1][0]) <= bQ).all() and (np.abs(outs[0][1] - outs[1][1]) <= bX).all()


def test_pass_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    S, W, Q, X = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(4))
    m = torch.eye(b, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for args in [(S, W, Q, Q), (S, S, Q, X), (X, W, Q, X), (S, W, W, X), (Q, W, Q, X)]:
        with pytest.raises(E):
            handle.bcg_update(m, m, *args)
    assert b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.bcg_direction(m, m, Q, Q)
    with pytest.raises(E):
        handle.bcg_update(m[:8], m, S, W, Q, X)
    with pytest.raises(E):
        handle.bcg_update(m.float(), m, S, W, Q, X)
    with pytest.raises(E):
        handle.bcg_update(m, m, S, W, Q, X[:, :8])
    big = [torch.zeros(n, 33, dtype=torch.float64, device="cuda") for _ in range(4)]
    m33 = torch.eye(33, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.bcg_update(m33, m33, *big)
    with pytest.raises(E):
        handle.bcg_direction(m33, m33, big[0], big[1])
    handle.bcg_update(m, m, S, W, Q, X)      # the calls after the errors succeed
    handle.bcg_direction(m, m, Q, S)


# ------------------------------------------------------------ 2. solves
REF = {}


def restated(lz, key, A, Bh, shift, tol, dtype):
    """bcg_restated once per case, shared by the tests that need it."""
    if key not in REF:
        REF[key] = bcg_restated(lz, A, Bh, shift=shift, tol=tol, dtype=dtype)
    return REF[key]


def solve_rhs(n, b, dtype):
    """fp64: the design's uniform [1, 2) columns.  fp32: test_gpu_cg's uniform (-1, 1) ones without
    the zero column.  A [1, 2) column is nearly the Laplacian's lowest mode, so |x| / |b| is about 1 /
    lambda_min (517 on the 100 x 100 grid) and the residual fp32 can hold, about eps32 |A| |x| / |b| =
    6e-8 x 8 x 517 = 2.5e-4, lies above the fp32 tolerance of 1e-4: such a case would test the number
    format, not the solver (the column method needs two restarts on it and ends at 0.90 tol).  A
    (-1, 1) column spreads over the modes and stays an order of magnitude clear of that floor."""
    return bcg_rhs(n, b) if dtype == F64 else lap_B(n, b, zero=None)


def check_block(lz, handle, torch, key, A, b, dtype, shift=0.0, tol=None, Bh=None, **kw):
    """Every check the design lists for a solve case; returns (out, Bh, the restatement)."""
    tol = TOL[dtype] if tol is None else tol
    eps, n = EPS[dtype], A.n
    Bh = (solve_rhs(n, b, dtype) if Bh is None else Bh).astype(dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, Bh)
    out = handle.solve(Ad, B, shift=shift, tol=tol, method="block", **kw)
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    Xh = f64(out["X"].cpu().numpy())
    assert np.isfinite(Xh).all()
    S, sg, B64 = sp_csr(A, F64), float(dtype(shift)), f64(Bh)
    r = np.linalg.norm(B64 - (S @ Xh + sg * Xh), axis=0)
    bn = np.linalg.norm(B64, axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    rnd = np.linalg.norm((nnz_row + 3) * eps * (abs(S) @ np.abs(Xh) + abs(sg) * np.abs(Xh) + np.abs(B64)), axis=0)
    ref = restated(lz, key, A, Bh, shift, tol, dtype)
    print(f"{key}: iters max {out['iters'].max()} (restated {ref['iters'].max()}), iterations {out['iterations']}, "
          f"restarts {out['restarts']} (restated {ref['restarts']}), n_spmm {out['n_spmm']}, fallback {out['fallback']} "
          f"(restated {ref['fallback']}), stop {out['stop']}, max resid/tol {(out['resid'] / tol).max():.3f}, "
          f"max true |r|/(tol |b|) {(r / np.maximum(tol * bn, 1e-300)).max():.3f}")
    assert out["converged"].all() and (out["status"] == MET).all(), f"status {out['status']}"
    assert (r <= tol * bn + rnd).all(), "the fp64 residual of the returned X"
    assert (np.abs(out["resid"] * bn - r) <= rnd + (n + 2) * EPS64 * r).all(), "resid against the recomputation"
    if dtype == F64:
        assert (out["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all(), "iterations against the restatement"
    else:
        assert (out["iters"] <= 2 * ref["iters"]).all(), "iterations against the restatement"
    if not out["fallback"]:
        assert out["stop"] == CONVERGED
        assert out["n_spmm"] == out["iterations"] + (2 + out["restarts"] if out["iterations"] else 1)
    return out, Bh, ref


@pytest.mark.parametrize("grid", [(40, 36), (7, 7), (100, 100)])
@pytest.mark.parametrize("b,dtype", HOT)
def test_solve_laplace(lz, handle, torch_cuda, b, dtype, grid):
    """(7, 7): 49 rows; the block Krylov space runs out and the columns finish one by one.  On the
    two larger grids in fp64 the design's condition: block iterations <= half of the column method's
    largest count, the column method run on the same device and right-hand sides."""
    A = lz.gen_laplace2d(*grid, dtype)
    out, Bh, _ = check_block(lz, handle, torch_cuda, f"laplace{grid} b={b} {dtype.__name__}", A, b, dtype)
    if grid == (7, 7) and b == 16:
        assert out["fallback"] == 1
    if grid != (7, 7):
        assert out["fallback"] == 0
        if dtype == F64:
            col = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, Bh), tol=TOL[dtype], method="columns")
            print(f"  columns: iters {col['iters'].min()}-{col['iters'].max()}; ratio "
                  f"{out['iters'].max() / col['iters'].max():.3f}")
            assert col["converged"].all() and 2 * out["iters"].max() <= col["iters"].max()


@pytest.mark.parametrize("b,dtype", HOT)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype):
    A = fused_operator(lz, "n1", dtype)
    assert A.n == 1
    out, *_ = check_block(lz, handle, torch_cuda, f"n1 b={b} {dtype.__name__}", A, b, dtype, shift=1.0)
    assert out["fallback"] == 1          # b > n


@pytest.mark.parametrize("name", ["n47", "n48", "n49", "n4099"])
@pytest.mark.parametrize("b,dtype", HOT)
def test_solve_shifted_banded(lz, handle, torch_cuda, b, dtype, name):
    A = fused_operator(lz, name, dtype)
    check_block(lz, handle, torch_cuda, f"{name} b={b} {dtype.__name__}", A, b, dtype, shift=gersh_shift(lz, A))


@pytest.mark.parametrize("b,dtype", GENERIC)
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype):
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    out, *_ = check_block(lz, handle, torch_cuda, f"banded1000 b={b} {dtype.__name__}", A, b, dtype,
                          shift=gersh_shift(lz, A))
    assert out["fallback"] == 0


def test_solve_generic_switch(lz, handle, torch_cuda, monkeypatch):
    """LZ_BCG_GENERIC=1 at b = 16 fp64: the same solve on the generic kernels."""
    A = lz.gen_laplace2d(40, 36)
    monkeypatch.setenv("LZ_BCG_GENERIC", "1")
    out, *_ = check_block(lz, handle, torch_cuda, "laplace(40, 36) b=16 float64", A, 16, F64)
    assert out["fallback"] == 0


# ------------------------------------------------------------ 3. semantics
@pytest.fixture(scope="module")
def lap(lz, handle, torch_cuda):
    """The 40 x 36 Laplacian at fp64, b = 16: the operator, its right-hand sides and one block solve."""
    class P:
        pass
    s = P()
    s.A = lz.gen_laplace2d(40, 36)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = bcg_rhs(s.A.n, 16)
    s.B = dev(torch_cuda, s.Bh)
    s.out = handle.solve(s.Ad, s.B, method="block")
    assert s.out["converged"].all() and s.out["fallback"] == 0
    return s


def test_result_keys(lz, lap, handle):
    col = handle.solve(lap.Ad, lap.B)
    base = {"X", "iters", "status", "converged", "resid", "est", "iterations", "restarts", "n_spmm"}
    assert set(col) == base and set(lap.out) == base | {"fallback", "stop"}


def test_columns_is_the_default(lz, lap, handle, torch_cuda):
    """method="columns" is what solve ran before: the default and the explicit form give the same
    bits, and the restatement of the column loop still describes them."""
    from test_cg_host import cg_restated
    d, c = handle.solve(lap.Ad, lap.B), handle.solve(lap.Ad, lap.B, method="columns")
    assert torch_cuda.equal(d["X"], c["X"]) and np.array_equal(d["iters"], c["iters"])
    assert np.array_equal(d["resid"], c["resid"]) and d["n_spmm"] == c["n_spmm"]
    ref = cg_restated(lz, lap.A, lap.Bh)
    assert d["converged"].all() and (d["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all()


def test_check_every(lz, lap, handle, torch_cuda):
    """The iterations enqueued behind a stop touch nothing: X and iters bit for bit."""
    outs = {k: handle.solve(lap.Ad, lap.B, method="block", check_every=k) for k in (1, 8, 16)}
    for k, o in outs.items():
        assert torch_cuda.equal(o["X"], lap.out["X"]) and np.array_equal(o["iters"], lap.out["iters"]), k
        assert np.array_equal(o["resid"], lap.out["resid"]) and np.array_equal(o["est"], lap.out["est"]), k
    assert outs[1]["iterations"] <= outs[8]["iterations"] < outs[1]["iterations"] + 8
    assert outs[1]["iterations"] <= outs[16]["iterations"] < outs[1]["iterations"] + 16


def test_reproducible(lz, lap, handle, torch_cuda):
    again = handle.solve(lap.Ad, lap.B, method="block")
    assert torch_cuda.equal(again["X"], lap.out["X"]) and np.array_equal(again["iters"], lap.out["iters"])
    assert np.array_equal(again["resid"], lap.out["resid"])


def test_converged_start(lz, lap, handle, torch_cuda):
    again = handle.solve(lap.Ad, lap.B, X0=lap.out["X"], method="block")
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], lap.out["X"]) and again["stop"] == CONVERGED


@pytest.mark.parametrize("kind", FALLBACKS)
def test_fallback(lz, handle, torch_cuda, kind):
    A, Bh = fallback_case(lz, kind)
    o = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, Bh), method="block")
    Xh = f64(o["X"].cpu().numpy())
    r = np.linalg.norm(Bh - sp_csr(A, F64) @ Xh, axis=0)
    print(f"{kind}: iters {o['iters'].tolist()}, iterations {o['iterations']}, n_spmm {o['n_spmm']}, stop {o['stop']}")
    assert o["fallback"] == 1 and o["stop"] == RANK and o["converged"].all()
    assert (r <= 1.05e-10 * np.linalg.norm(Bh, axis=0)).all()
    if kind == "zero":
        assert (o["X"][:, 3] == 0).all() and o["resid"][3] == 0 and o["iters"][3] == 0
    Ad, B = lz.CsrDevice.from_host(A), dev(torch_cuda, Bh)
    if kind == "7x7":
        # exactly three block iterations, then the guard: held to three the block runs them all and
        # ends spent without a fallback; allowed a fourth it does not run it but hands over
        o3 = handle.solve(Ad, B, method="block", max_iter=3)
        assert (o3["iters"] == 3).all() and o3["fallback"] == 0 and o3["stop"] == R_SPENT
        o4 = handle.solve(Ad, B, method="block", max_iter=4)
        assert o4["fallback"] == 1 and o4["stop"] == RANK and (o4["iters"] <= 4).all()
    else:
        # no block iteration ran: the first start tripped the guard, so the column solver started
        # from the untouched X0 with every iteration left -- its own result, bit for bit
        col = handle.solve(Ad, B, method="columns")
        assert torch_cuda.equal(o["X"], col["X"]) and np.array_equal(o["iters"], col["iters"])
        assert o["iterations"] == col["iterations"] and o["n_spmm"] == col["n_spmm"] + 1


def test_scaled_columns(lz, lap, handle, torch_cuda):
    Bh = lap.Bh * 10.0 ** np.linspace(-8, 8, 16)
    o = handle.solve(lap.Ad, dev(torch_cuda, Bh), method="block")
    r = np.linalg.norm(Bh - sp_csr(lap.A, F64) @ f64(o["X"].cpu().numpy()), axis=0) / np.linalg.norm(Bh, axis=0)
    print(f"scaled columns: iters {o['iters'].max()}, restarts {o['restarts']}, max |r|/|b| {r.max():.3e}")
    assert o["converged"].all() and o["fallback"] == 0 and (r <= 1.05e-10).all()


def test_not_positive_definite(lz, lap, handle, torch_cuda):
    X0 = dev(torch_cuda, np.random.default_rng(1).uniform(-1, 1, lap.Bh.shape))
    keep = X0.clone()
    o = handle.solve(lap.Ad, lap.B, shift=-1.0, X0=X0, method="block")
    assert (o["status"] == NOT_PD).all() and o["stop"] == R_NOT_PD and o["fallback"] == 0
    assert torch_cuda.equal(o["X"], keep) and torch_cuda.equal(X0, keep), "X equals X0 bit for bit"
    assert not o["converged"].any() and (o["iters"] == 0).all()


def test_unreachable_tol(lz, handle, torch_cuda):
    A = lz.gen_laplace2d(40, 36, F32)
    Bh = bcg_rhs(A.n, 32).astype(F32)
    Ad = lz.CsrDevice.from_host(A)
    o = handle.solve(Ad, dev(torch_cuda, Bh), tol=1e-9, method="block")
    print(f"fp32 at tol 1e-9: restarts {o['restarts']}, iters max {o['iters'].max()}, resid {o['resid'].max():.3e}, "
          f"fallback {o['fallback']}")
    assert not o["converged"].any() and (o["status"] == SPENT).all() and torch_cuda.isfinite(o["X"]).all()
    assert o["fallback"] == 0 and o["restarts"] == 3
    o1 = handle.solve(Ad, dev(torch_cuda, Bh), tol=1e-9, max_restarts=1, method="block")
    assert o1["restarts"] == 1 and o1["fallback"] == 0 and (o1["status"] == SPENT).all()


def test_max_iter(lz, handle, torch_cuda):
    A = lz.gen_laplace2d(100, 100)
    o = handle.solve(lz.CsrDevice.from_host(A), dev(torch_cuda, bcg_rhs(A.n, 16)), max_iter=5, method="block")
    assert (o["status"] == SPENT).all() and (o["iters"] == 5).all() and o["stop"] == R_SPENT
    assert o["restarts"] == 0 and o["fallback"] == 0 and torch_cuda.isfinite(o["X"]).all()
    assert o["n_spmm"] == o["iterations"] + 2 and o["iterations"] == 8      # one chunk of check_every = 8


def test_arguments(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = lap.A.n, 16
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, method="blocks")                     # unknown method
    with pytest.raises(E):
        handle.solve(lap.Ad, torch.zeros(n, 33, dtype=torch.float64, device="cuda"), method="block")
    handle.solve(lap.Ad, torch.ones(n, 33, dtype=torch.float64, device="cuda"), max_iter=1)   # columns: b <= 64
    with pytest.raises(E):
        handle.solve(lap.Ad, lap.B, tol=0.0, method="block")
    with pytest.raises(E):
        handle.solve(lz.CsrDevice.from_host(lap.A, n_cols=n + 1), lap.B, method="block")
    buf = torch.zeros(6 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):                                               # work holds B
        handle.solve(lap.Ad, buf[n * b:2 * n * b].view(n, b), work=buf[:4 * n * b], method="block")
    p = lambda t: t.data_ptr()
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    iters, status, info = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(5, np.int32)
    resid, est = np.zeros(b), np.zeros(b)

    def raw(Bt, Xp, workp, bb=b):
        return handle.L.lz_bcg_solve(handle.ptr, n, lap.A.nnz, p(lap.Ad.row_ptr), p(lap.Ad.col), p(lap.Ad.val),
                                     lz.LZ_F64, bb, 0.0, p(Bt), Xp, workp, ctypes.addressof(opts), lz._p(iters),
                                     lz._p(status), lz._p(resid), lz._p(est), lz._p(info))
    Xt = torch.zeros(n, b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        lz._check(raw(lap.B, p(lap.B), p(buf)), "X aliases B")
    with pytest.raises(E):
        lz._check(raw(lap.B, p(buf) + 8 * n * b, p(buf)), "work holds X")
    with pytest.raises(E):
        lz._check(raw(lap.B, p(Xt), p(buf), bb=33), "b > 32")
    assert b"argument error" in handle.L.lz_last_error()
    lz._check(raw(lap.B, p(Xt), p(buf)), "lz_bcg_solve")                # the call after the errors succeeds
    assert torch.equal(lap.B, dev(torch, lap.Bh)), "B is read only"
    assert info[3] == 0 and info[4] == R_SPENT and (iters == 10).all()      # (opts: max_iter 10)
