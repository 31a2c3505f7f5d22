"""Diagonally preconditioned conjugate gradients on the device: lz_pcg_update (both forms of
k_cg_update with PRE), lz_csr_jacobi and Handle.solve(precond=...) (lz_pcg_solve).

pcg_update: test_gpu_cg's forward bounds with z0 = dv r in P's expression, extended to Z (3 eps of
dv r' plus dv times R's bound); both dots against the device's own R and Z.  jacobi: the fp64
definition, summed in the order of the positions.  solve: test_gpu_cg's checks with the
restatement of test_pcg_host as the yardstick for the iteration counts.
"""
import ctypes
import math

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT, gersh_shift, sp_csr
from test_gpu_cg import EPS, EPS64, F32, F64, FORM128, TOL, dev, f64, rhs, update_inputs, update_rows
from test_gpu_cheb import fused_operator
from test_pcg_host import TABLE, graphlap, jacobi_host, pcg_restated, table_run

pytestmark = pytest.mark.gpu

GENERIC = [(1, F64), (5, F64), (8, F64), (16, F32), (64, F32)]


# ------------------------------------------------------------ 1. pcg_update
def pupdate_inputs(n, b, dtype, seed, unit=False):
    blocks, coef, zc, fc = update_inputs(n, b, dtype, seed)
    dinv = np.ones(n, dtype) if unit else np.random.default_rng(seed + 77).uniform(0.5, 2.0, n).astype(dtype)
    return blocks, dinv, coef, zc, fc


def run_pupdate(handle, torch, n, b, dtype, seed, unit=False):
    blocks, dinv, coef, zc, fc = pupdate_inputs(n, b, dtype, seed, unit)
    R, W, P, S, X = (dev(torch, a) for a in blocks)
    Z = torch.full_like(R, float("nan"))  # written, never read
    cf, dv = dev(torch, coef), dev(torch, dinv)
    dots = torch.full((2 * b,), float("nan"), dtype=torch.float64, device="cuda")
    handle.pcg_update(cf, dv, R, W, P, S, X, Z, dots=dots)
    return blocks, dinv, coef, zc, fc, (R, W, P, S, X, Z), cf, dv, dots


def check_pupdate(lz, handle, torch, n, b, dtype, seed=0):
    (Rh, Wh, Ph, Sh, Xh), dinv, coef, zc, fc, (R, W, P, S, X, Z), cf, dvt, dots = run_pupdate(handle, torch, n, b,
                                                                                           dtype, seed)
    eps, what = EPS[dtype], f"n={n} b={b} {dtype.__name__}"
    al, be = f64(coef[:b].astype(dtype)), f64(coef[b:].astype(dtype))
    r, w, x, dv = f64(Rh), f64(Wh), f64(Xh), f64(dinv)[:, None]
    p, s = np.where(be == 0, 0.0, f64(Ph)), np.where(be == 0, 0.0, f64(Sh))  # beta == 0: not used
    z0 = dv * r
    p1, s1 = be * p + z0, be * s + w
    x1, r1 = al * p1 + x, -al * s1 + r
    z1 = dv * r1
    dP = 3 * eps * (np.abs(be * p) + np.abs(z0))
    dS = 3 * eps * (np.abs(be * s) + np.abs(w))
    dX = 3 * eps * (np.abs(al * p1) + np.abs(x)) + np.abs(al) * dP
    dR = 3 * eps * (np.abs(al * s1) + np.abs(r)) + np.abs(al) * dS
    dZ = 3 * eps * np.abs(z1) + dv * dR
    got = {k: f64(t.cpu().numpy()) for k, t in (("P", P), ("S", S), ("X", X), ("R", R), ("Z", Z))}
    worst = 0.0
    for k, ref, bound in (("P", p1, dP), ("S", s1, dS), ("X", x1, dX), ("R", r1, dR), ("Z", z1, dZ)):
        assert np.isfinite(got[k]).all(), f"{what}: NaN / Inf in {k}"
        err = np.abs(got[k] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"{what}: {k}"
    assert torch.equal(W, dev(torch, Wh)) and torch.equal(cf, dev(torch, coef)) and torch.equal(dvt, dev(torch, dinv)), \
        f"{what}: W / coef / dinv are read only"
    scaled = lambda c: dev(torch, dinv * Rh[:, c])  # one rounded product in the dtype
    if zc is not None:
        assert torch.equal(X[:, zc], dev(torch, Xh[:, zc])) and torch.equal(R[:, zc], dev(torch, Rh[:, zc])), \
            f"{what}: alpha = beta = 0 leaves X and R bit for bit"
        assert torch.equal(Z[:, zc], scaled(zc)), f"{what}: a frozen column's Z is dv r, the same bits again"
    if fc is not None:
        assert torch.equal(P[:, fc], scaled(fc)) and torch.equal(S[:, fc], dev(torch, Wh[:, fc]))
    dh = dots.cpu().numpy()
    assert np.isfinite(dh).all(), f"{what}: NaN in dots"
    for name, gotd, terms in (("r.z", dh[:b], got["R"] * got["Z"]), ("r.r", dh[b:], got["R"] ** 2)):
        ref, mag = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        derr = np.abs(gotd - ref)
        print(f"{what}: {name} max err/bound {(derr / np.maximum((n + 2) * EPS64 * mag, 1e-300)).max():.3e}")
        assert (derr <= (n + 2) * EPS64 * mag).all(), f"{what}: {name}"
    print(f"{what}: max err/bound {worst:.3f}")
    return R, P, S, X, Z, dots


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_update_parity(lz, handle, torch_cuda, b, dtype):
    rpb, rows = update_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) > lz.CG_GRID_CAP and math.ceil(rows[-2] / rpb) == 257
    for n in rows:
        check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
    if b == 1:  # both kinds of its one column
        for seed in (2, 3):
            check_pupdate(lz, handle, torch_cuda, rows[3], b, dtype, seed=seed)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
def test_unit_dinv_is_cg_update(lz, handle, torch_cuda, monkeypatch, b, dtype, generic):
    """dinv = 1: P, S, X, R are lz_cg_update's bits, Z is R, and r.z is r.r bit for bit."""
    torch = torch_cuda
    if generic:
        monkeypatch.setenv("LZ_CG_GENERIC", "1")
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        blocks, _, coef, *_, (R, W, P, S, X, Z), cf, dv, dots = run_pupdate(handle, torch, n, b, dtype, 7, unit=True)
        R0, W0, P0, S0, X0 = (dev(torch, a) for a in blocks)
        handle.cg_update(dev(torch, coef), R0, W0, P0, S0, X0)
        for k, u, v in zip("RPSX", (R, P, S, X), (R0, P0, S0, X0)):
            assert torch.equal(u, v), f"n={n}: {k} differs from lz_cg_update's"
        assert torch.equal(Z, R) and torch.equal(dots[:b], dots[b:])


@pytest.mark.parametrize("b,dtype", FORM128)
def test_update_forms_agree(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """Both forms finish every element with the same operations: the same bits in the five blocks
    (the dots sum in another order: each within its bound, above); the store flavours change no bit."""
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        fast = check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        again = check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for u, v in zip(fast, again):
            assert torch_cuda.equal(u, v), "two runs: every bit, the dots included"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_GENERIC", "1")
            gen = check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
            gen2 = check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for k, u, v in zip("RPSXZ", fast[:5], gen[:5]):
            assert torch_cuda.equal(u, v), f"n={n}: {k} differs between the forms"
        assert torch_cuda.equal(gen[5], gen2[5]), "two runs of the generic form: the same dots"
        for var, val in (("LZ_CG_NT", "0"), ("LZ_PCG_Z_NT", "0")):
            with monkeypatch.context() as mp:
                mp.setenv(var, val)
                other = check_pupdate(lz, handle, torch_cuda, n, b, dtype, seed=7)
            for u, v in zip(fast, other):
                assert torch_cuda.equal(u, v), f"{var}={val}: every bit, the dots included"


def test_update_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b = 40, 16
    R, W, P, S, X, Z = (torch.zeros(n, b, dtype=torch.float64, device="cuda") for _ in range(6))
    cf = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
    dv = torch.ones(n, dtype=torch.float64, device="cuda")
    E = lz.LanczosError
    for args in [(R, W, P, S, X, R), (R, W, P, S, X, X), (R, R, P, S, X, Z), (R, W, P, P, X, Z), (X, W, P, S, X, Z),
                 (R, W, P, S, Z, Z)]:
        with pytest.raises(E):
            handle.pcg_update(cf, dv, *args)
    with pytest.raises(E):                      # dinv inside a block
        handle.pcg_update(cf, Z.view(-1)[:n], R, W, P, S, X, Z)
    assert b"argument error" in handle.L.lz_last_error()
    with pytest.raises(E):
        handle.pcg_update(cf[:b], dv, R, W, P, S, X, Z)
    with pytest.raises(E):
        handle.pcg_update(cf, dv[:n - 1], R, W, P, S, X, Z)
    with pytest.raises(E):
        handle.pcg_update(cf, dv, R, W, P, S, X, Z[:, :8])
    big = [torch.zeros(n, 65, dtype=torch.float64, device="cuda") for _ in range(6)]
    with pytest.raises(E):
        handle.pcg_update(torch.zeros(130, dtype=torch.float64, device="cuda"), dv, *big)
    assert b"argument error" in handle.L.lz_last_error()
    p = lambda t: t.data_ptr()
    dots = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
    for k in range(9):                          # each pointer NULL in turn
        ptrs = [p(cf), p(dv), p(R), p(W), p(P), p(S), p(X), p(Z), p(dots)]
        ptrs[k] = None
        assert handle.L.lz_pcg_update(handle.ptr, n, b, lz.LZ_F64, *ptrs) != 0
        assert b"argument error" in handle.L.lz_last_error()
    handle.pcg_update(cf, dv, R, W, P, S, X, Z)  # the call after the errors succeeds


# ------------------------------------------------------------ 2. jacobi
def jacobi_ref(n, rp, col, val, shift, dtype):
    """d_i in fp64: the row's diagonal entries added in the order of their positions (np.add.at
    applies them one by one in index order), then the shift rounded once to the dtype."""
    rows = np.repeat(np.arange(n), np.diff(rp))
    on = col == rows
    d = np.zeros(n)
    np.add.at(d, rows[on], val[on].astype(dtype).astype(F64))
    return d + float(dtype(shift))


def jacobi_raw(lz, handle, torch, n, rp, col, val, shift, dtype):
    A = lz.CsrDevice(n, n, dev(torch, rp.astype(np.int64)), dev(torch, col.astype(np.int32)), dev(torch, val.astype(dtype)))
    out = []
    for _ in range(2):
        dinv = torch.full((n,), float("nan"), dtype=A.val.dtype, device="cuda")
        bad = ctypes.c_int64(-1)
        lz._check(handle.L.lz_csr_jacobi(handle.ptr, n, A.nnz, A.row_ptr.data_ptr(), A.col.data_ptr(), A.val.data_ptr(),
                                         A.dtype, float(shift), dinv.data_ptr(), ctypes.addressof(bad)), "lz_csr_jacobi")
        out.append((dinv, bad.value))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1], "two runs: the same bits"
    return A, out[0][0].cpu().numpy(), out[0][1]


def check_jacobi(lz, handle, torch, n, rp, col, val, shift, dtype, bad_rows=()):
    A, got, n_bad = jacobi_raw(lz, handle, torch, n, rp, col, val, shift, dtype)
    d = jacobi_ref(n, rp, col, val, shift, dtype)
    good = np.ones(n, bool)
    good[list(bad_rows)] = False
    assert n_bad == len(bad_rows) and (got[~good] == 0).all(), f"n_bad {n_bad}, planted {len(bad_rows)}"
    ref = 1.0 / d[good]
    # one rounding of the dtype (half an ulp of the exact quotient) and the fp64 division's own
    err = np.abs(f64(got[good]) - ref)
    assert (err <= (0.5 * EPS[dtype] + 2 * EPS64) * np.abs(ref)).all(), f"n={n} {dtype.__name__}: max {err.max():.3e}"
    return A


def random_rows(n, per_row, seed):
    """per_row entries a row, the diagonal among them at a random position, columns unsorted."""
    rng = np.random.default_rng(seed)
    rp = np.arange(n + 1, dtype=np.int64) * per_row
    col = rng.integers(0, n, n * per_row).astype(np.int32)
    val = rng.uniform(0.5, 2.0, n * per_row)
    rows = np.arange(n)
    col[rows * per_row + rng.integers(0, per_row, n)] = rows
    return rp, col, val


@pytest.mark.parametrize("dtype", [F64, F32])
def test_jacobi_small_shapes(lz, handle, torch_cuda, dtype):
    check_jacobi(lz, handle, torch_cuda, 1, np.array([0, 1]), np.array([0]), np.array([2.0]), 0.0, dtype)
    # n one under, at and over the rows of a workgroup pass, and two passes and a row
    for n in (lz.JACOBI_ROWS - 1, lz.JACOBI_ROWS, lz.JACOBI_ROWS + 1, 2 * lz.JACOBI_ROWS + 1):
        rp, col, val = random_rows(n, 3, n)
        check_jacobi(lz, handle, torch_cuda, n, rp, col, val, 0.25, dtype)
    # row 0 empty, row 1 without a stored diagonal, row 2 a diagonal alone, row 3 empty (shift > 0)
    rp, col, val = np.array([0, 0, 2, 3, 3]), np.array([0, 3, 2]), np.array([5.0, 7.0, 3.0])
    check_jacobi(lz, handle, torch_cuda, 4, rp, col, val, 0.5, dtype)
    # nnz = 0
    check_jacobi(lz, handle, torch_cuda, 3, np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), 2.0, dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_jacobi_long_rows_and_duplicates(lz, handle, torch_cuda, dtype):
    """graphlap(4096, cap=512) (the longest row well past one pass of a row's lanes) with row 17 replaced
    by 5000 unsorted entries, four of them on the diagonal: 1e16, 3, -1e16, 5 at positions far apart,
    whose sum depends on the order (7 or 9 in the order of the positions; 8 in any other)."""
    G = graphlap(lz, 4096, 512, dtype)
    deg = np.diff(G.row_ptr)
    assert deg.max() > 8 * lz.JACOBI_LANES
    r, m = 17, 5000
    rng = np.random.default_rng(11)
    ncol = rng.integers(0, G.n, m).astype(np.int32)
    ncol[ncol == r] = r + 1
    nval = rng.uniform(-1, 1, m)
    for pos, v in zip((3, 1000, 2500, 4999), (1e16, 3.0, -1e16, 5.0)):
        ncol[pos], nval[pos] = r, v
    a, e = G.row_ptr[r], G.row_ptr[r + 1]
    col = np.concatenate([G.col[:a], ncol, G.col[e:]])
    val = np.concatenate([G.val[:a].astype(F64), nval, G.val[e:].astype(F64)])
    rp = G.row_ptr.copy()
    rp[r + 1:] += m - (e - a)
    d = jacobi_ref(G.n, rp, col, val, 1.0, dtype)
    assert d[r] in (8.0, 10.0)  # 7 or 9, and the shift
    check_jacobi(lz, handle, torch_cuda, G.n, rp, col, val, 1.0, dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_jacobi_counts_bad_rows(lz, handle, torch_cuda, dtype):
    n = 70
    rp, col, val = random_rows(n, 3, 5)
    col[15:18] = (6, 7, 8)                                # row 5: no stored diagonal, shift 0: d = 0
    col[120:123], val[120] = (40, 41, 42), -1.0           # row 40: negative
    col[207:210], val[207] = (69, 1, 2), np.nan           # row 69: NaN
    A = check_jacobi(lz, handle, torch_cuda, n, rp, col, val, 0.0, dtype, bad_rows=(5, 40, 69))
    with pytest.raises(lz.LanczosError, match="3 rows"):
        handle.jacobi(A)
    # the same rows with a shift that mends row 5 alone
    check_jacobi(lz, handle, torch_cuda, n, rp, col, val, 0.5, dtype, bad_rows=(40, 69))
    rp, col, val = random_rows(n, 3, 5)
    A = check_jacobi(lz, handle, torch_cuda, n, rp, col, val, 0.0, dtype)
    got = handle.jacobi(A)
    assert got.dtype == A.val.dtype and tuple(got.shape) == (n,) and (got > 0).all()


# ------------------------------------------------------------ 3. solve
REF = {}


def check_psolve(lz, handle, torch, key, A, b, dtype, shift=0.0, tol=None, ref=None, precond="jacobi", **kw):
    """test_gpu_cg.check_solve for the preconditioned solve; returns (out, Bh, the SpMM kernel id)."""
    tol = TOL[dtype] if tol is None else tol
    eps, n = EPS[dtype], A.n
    Bh = rhs(n, b, dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, Bh)
    out = handle.solve(Ad, B, shift=shift, tol=tol, precond=precond, **kw)
    kernel = handle.last_kernel()[0]
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    assert out["precond"] == (precond if isinstance(precond, str) else "diagonal")
    Xh = f64(out["X"].cpu().numpy())
    assert np.isfinite(Xh).all()
    S, sg, B64 = sp_csr(A, F64), float(dtype(shift)), f64(Bh)
    r = np.linalg.norm(B64 - (S @ Xh + sg * Xh), axis=0)
    bn = np.linalg.norm(B64, axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    rnd = np.linalg.norm((nnz_row + 3) * eps * (abs(S) @ np.abs(Xh) + abs(sg) * np.abs(Xh) + np.abs(B64)), axis=0)
    if ref is None:
        if key not in REF:
            REF[key] = pcg_restated(lz, A, Bh, jacobi_host(A, shift, dtype), shift=shift, tol=tol, dtype=dtype)
        ref = REF[key]
    print(f"{key}: iters max {out['iters'].max()} (restated {ref['iters'].max()}), iterations {out['iterations']}, "
          f"restarts {out['restarts']} (restated {ref['restarts']}), n_spmm {out['n_spmm']}, max resid/tol "
          f"{(out['resid'] / tol).max():.3f}, max true |r|/(tol |b|) {(r / np.maximum(tol * bn, 1e-300)).max():.3f}")
    print(f"  device iters   {out['iters'].tolist()}\n  restated iters {ref['iters'].tolist()}")
    assert out["converged"].all() and (out["status"] == MET).all(), f"status {out['status']}"
    assert (r <= tol * bn + rnd).all(), "the fp64 residual of the returned X"
    assert (np.abs(out["resid"] * bn - r) <= rnd + (n + 2) * EPS64 * r).all(), "resid against the recomputation"
    if out["restarts"] == 0:
        assert (out["est"] <= tol).all(), "the recurrence's last value froze the column"
    if dtype == F64:
        assert (out["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all(), "iterations against the restatement"
    else:
        assert (out["iters"] <= 2 * ref["iters"]).all(), "iterations against the restatement"
    assert out["n_spmm"] == out["iterations"] + (2 + out["restarts"] if out["iterations"] else 1)
    return out, Bh, kernel


@pytest.mark.parametrize("name", ["varcoef7x7", "varcoef40x36", "reaction100x100", "graphlap4096"])
@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_jacobi(lz, handle, torch_cuda, b, dtype, name):
    """The operators Jacobi is for (varcoef7x7: 49 rows, one past the fused SpMM's 48-row tile);
    128-byte rows, so the SpMM under the solve is the fused one with its dots."""
    make, args, shift = TABLE[name]
    A = make(lz, *args, dtype=dtype)
    *_, kernel = check_psolve(lz, handle, torch_cuda, f"{name} b={b} {dtype.__name__}", A, b, dtype, shift=shift,
                              ref=table_run(lz, name, dtype, True))
    assert kernel & lz.LZ_K_DOT, f"kernel id {kernel:#x}"


@pytest.mark.parametrize("b,dtype", FORM128)
def test_solve_one_row(lz, handle, torch_cuda, b, dtype):
    A = fused_operator(lz, "n1", dtype)
    assert A.n == 1
    check_psolve(lz, handle, torch_cuda, f"n1 b={b} {dtype.__name__}", A, b, dtype, shift=1.0)


@pytest.mark.parametrize("b,dtype", [(1, F64), (5, F64), (64, F32)])
def test_solve_generic_b(lz, handle, torch_cuda, b, dtype):
    """A near-constant diagonal: Jacobi only has to be correct here."""
    A = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=dtype)
    *_, kernel = check_psolve(lz, handle, torch_cuda, f"banded1000 b={b} {dtype.__name__}", A, b, dtype,
                              shift=gersh_shift(lz, A))
    assert not kernel & lz.LZ_K_DOT


@pytest.mark.parametrize("b,dtype", FORM128)
def test_callers_dinv(lz, handle, torch_cuda, b, dtype):
    """A caller's tensor equal to Handle.jacobi's gives the bits of precond="jacobi"."""
    make, args, shift = TABLE["graphlap4096"]
    A = make(lz, *args, dtype=dtype)
    Ad, B = lz.CsrDevice.from_host(A), dev(torch_cuda, rhs(A.n, b, dtype))
    dinv = handle.jacobi(Ad, shift)
    o1 = handle.solve(Ad, B, shift=shift, precond="jacobi")
    o2 = handle.solve(Ad, B, shift=shift, precond=dinv.clone())
    assert o1["precond"] == "jacobi" and o2["precond"] == "diagonal"
    assert torch_cuda.equal(o1["X"], o2["X"]) and np.array_equal(o1["iters"], o2["iters"])
    assert np.array_equal(o1["resid"], o2["resid"]) and np.array_equal(o1["est"], o2["est"])


# ------------------------------------------------------------ 4. semantics
@pytest.fixture(scope="module")
def pre(lz, handle, torch_cuda):
    """varcoef(40, 36, 1e4) at fp64, b = 16: the operator, its right-hand sides and one Jacobi solve."""
    class P:
        pass
    s = P()
    s.A = TABLE["varcoef40x36"][0](lz, 40, 36, 1e4)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.out = handle.solve(s.Ad, s.B, precond="jacobi")
    assert s.out["converged"].all() and s.out["restarts"] == 0
    return s


def test_zero_column(lz, pre, torch_cuda):
    o = pre.out
    assert o["iters"][3] == 0 and o["status"][3] == MET and o["resid"][3] == 0 and o["est"][3] == 0
    assert (o["X"][:, 3] == 0).all()
    assert torch_cuda.isfinite(o["X"]).all() and np.isfinite(o["resid"]).all() and np.isfinite(o["est"]).all()


def test_converged_start(lz, pre, handle, torch_cuda):
    again = handle.solve(pre.Ad, pre.B, X0=pre.out["X"], precond="jacobi")
    assert (again["iters"] == 0).all() and again["iterations"] == 0 and again["n_spmm"] == 1
    assert again["converged"].all() and torch_cuda.equal(again["X"], pre.out["X"])
    assert np.array_equal(again["resid"], pre.out["resid"])


@pytest.mark.parametrize("j", [5, 15])
def test_independent_columns(lz, pre, handle, torch_cuda, j):
    B2h = np.repeat(pre.Bh[:, :1], 16, axis=1)
    B2h[:, j] = pre.Bh[:, j]
    o2 = handle.solve(pre.Ad, dev(torch_cuda, B2h), precond="jacobi")
    assert o2["restarts"] == 0
    assert torch_cuda.equal(o2["X"][:, j], pre.out["X"][:, j]) and o2["iters"][j] == pre.out["iters"][j]
    assert o2["resid"][j] == pre.out["resid"][j]


def test_check_every_and_reproducible(lz, pre, handle, torch_cuda):
    o1, o7 = (handle.solve(pre.Ad, pre.B, check_every=k, precond="jacobi") for k in (1, 7))
    assert torch_cuda.equal(o1["X"], o7["X"]) and np.array_equal(o1["iters"], o7["iters"])
    assert torch_cuda.equal(o1["X"], pre.out["X"]) and np.array_equal(o1["iters"], pre.out["iters"])
    assert o1["iterations"] <= o7["iterations"] < o1["iterations"] + 7


def test_max_iter(lz, pre, handle, torch_cuda):
    o = handle.solve(pre.Ad, pre.B, max_iter=5, precond="jacobi")
    nz = np.arange(16) != 3
    assert (o["status"][nz] == SPENT).all() and o["iters"].max() == 5 and (o["iters"][nz] == 5).all()
    assert o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()


def test_not_positive_definite(lz, handle, torch_cuda):
    """The Laplacian - 9 I is negative definite: Handle.jacobi refuses its diagonal, and a positive
    dinv of the caller's ends every nonzero column with status 2, X untouched."""
    torch = torch_cuda
    A = lz.gen_laplace2d(40, 36)
    Ad, Bh = lz.CsrDevice.from_host(A), rhs(A.n, 16, F64)
    with pytest.raises(lz.LanczosError, match="1440 rows"):
        handle.solve(Ad, dev(torch, Bh), shift=-9.0, precond="jacobi")
    X0 = dev(torch, np.random.default_rng(1).uniform(-1, 1, Bh.shape))
    X0[:, 3] = 0
    keep = X0.clone()
    o = handle.solve(Ad, dev(torch, Bh), shift=-9.0, X0=X0, precond=torch.full((A.n,), 0.25, dtype=torch.float64,
                                                                             device="cuda"))
    nz = np.arange(16) != 3
    assert (o["status"][nz] == NOT_PD).all() and (o["iters"] == 0).all() and o["status"][3] == MET
    assert torch.equal(o["X"], keep) and not o["converged"][nz].any()


def test_negative_dinv_is_status_2(lz, pre, handle, torch_cuda):
    """A preconditioner that is not positive on the residual: r.z <= 0, status 2."""
    o = handle.solve(pre.Ad, pre.B, precond=-handle.jacobi(pre.Ad))
    nz = np.arange(16) != 3
    assert (o["status"][nz] == NOT_PD).all() and (o["iters"] == 0).all() and (o["X"] == 0).all()


def test_arguments_and_default_path(lz, pre, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = pre.A.n, 16
    with pytest.raises(E):
        handle.solve(pre.Ad, pre.B, method="block", precond="jacobi")
    with pytest.raises(E):
        handle.solve(pre.Ad, pre.B, precond="ilu")
    buf = torch.zeros(5 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.solve(pre.Ad, pre.B, precond="jacobi", work=buf[:4 * n * b])   # work too small
    dinv = handle.jacobi(pre.Ad)
    with pytest.raises(E):
        handle.solve(pre.Ad, pre.B, precond=dinv[:n - 1])
    with pytest.raises(E):
        handle.solve(pre.Ad, pre.B, precond=dinv.float())
    with pytest.raises(E):                                                    # dinv inside work
        handle.solve(pre.Ad, pre.B, precond=buf[:n], work=buf)
    assert b"argument error" in handle.L.lz_last_error()
    # dinv NULL at the C entry point: an error, never a plain solve
    p = lambda t: t.data_ptr()
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    iters, status, info = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(3, np.int32)
    resid, est = np.zeros(b), np.zeros(b)
    Xt = torch.zeros(n, b, dtype=torch.float64, device="cuda")
    rc = handle.L.lz_pcg_solve(handle.ptr, n, pre.A.nnz, p(pre.Ad.row_ptr), p(pre.Ad.col), p(pre.Ad.val), lz.LZ_F64, b,
                               0.0, None, p(pre.B), p(Xt), p(buf), ctypes.addressof(opts), lz._p(iters), lz._p(status),
                               lz._p(resid), lz._p(est), lz._p(info))
    assert rc != 0 and b"argument error" in handle.L.lz_last_error() and (Xt == 0).all()
    ok = handle.solve(pre.Ad, pre.B, precond="jacobi", work=buf)              # the call after the errors succeeds
    assert torch.equal(ok["X"], pre.out["X"])
    # precond=None is the call without the argument, bit for bit
    plain, none = handle.solve(pre.Ad, pre.B, max_iter=200), handle.solve(pre.Ad, pre.B, max_iter=200, precond=None)
    assert plain.get("precond") is None and set(plain) == set(none) == set(pre.out) - {"precond"}
    assert torch.equal(plain["X"], none["X"]) and np.array_equal(plain["iters"], none["iters"])
