"""Multi-shift conjugate gradients on the device: lz_mscg_update (both forms of k_mscg_update) and
Handle.solve_shifts (lz_mscg_solve).

mscg_update: each of P_k, X_k, S, R elementwise against the fp64 evaluation of the documented
order, within 3 eps(dtype) x (the sum of the absolute values of that expression's terms), the
error of the new P_k and S carried into X_k's and R's bounds (test_gpu_cg.check_update's
derivation; t = zeta r is one more rounding inside P's three); rr against the device's own R with
that file's reduction bound.  solve_shifts: the NumPy fp64 residual of every returned X_k, the
returned resid, and the iteration counts against test_mscg_host's restatement of the two phases.
"""
import math

import numpy as np
import pytest

from test_cg_host import MET, NOT_PD, SPENT
from test_gpu_cg import EPS, EPS64, F32, F64, FORM128, GENERIC, TOL, dev, f64, update_inputs, update_rows
from test_mscg_host import CASES, SHIFT_LISTS, finishing_cap, operator, restated, rhs

pytestmark = pytest.mark.gpu


def bits(t):
    """The tensor's bit patterns: equality that takes NaN for what it is."""
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(torch, u, v):
    return torch.equal(bits(u), bits(v))


# ------------------------------------------------------------ 1. mscg_update
def mscg_inputs(n, b, dtype, s, seed, live=None):
    """R, W, S (n, b), P, X (s, n, b), coef and per shift the column with a_k = 0 (its P_k NaN: kept
    bit for bit) and the one with b_k = 0 (its P_k NaN: p' = t); the seed's frozen column (alpha =
    beta = 0).  b = 1: the only column takes one kind per call, by seed % 3."""
    rng = np.random.default_rng(seed)
    R, W, S = (rng.uniform(-1, 1, (n, b)).astype(dtype) for _ in range(3))
    P, X = (rng.uniform(-1, 1, (s, n, b)).astype(dtype) for _ in range(2))
    coef = rng.uniform(-2, 2, (2 + 3 * s) * b)
    coef[np.abs(coef) < 1e-3] = 0.5
    ac, fc = [None] * s, [None] * s
    zc = b // 2 if b > 1 else None
    if zc is not None:
        coef[zc] = coef[b + zc] = 0.0
    for k in range(s):
        o = (2 + 3 * k) * b
        if b > 1:
            ac[k], fc[k] = (b // 2 + 1 + k) % b, (b // 2 + 2 + k) % b
        elif seed % 3 == 1:
            ac[k] = 0
        elif seed % 3 == 2:
            fc[k] = 0
        if ac[k] is not None:
            coef[o + b + ac[k]] = 0.0
            P[k][:, ac[k]] = np.nan
        if fc[k] is not None and fc[k] != ac[k]:
            coef[o + 2 * b + fc[k]] = 0.0
            P[k][:, fc[k]] = np.nan
        else:
            fc[k] = None
    live = np.ones(s, np.int32) if live is None else np.asarray(live, np.int32)
    return (R, W, S, P, X), coef, live, zc, ac, fc


def run_mscg(handle, torch, host):
    (Rh, Wh, Sh, Ph, Xh), coef, live = host[:3]
    R, W, S, P, X = (dev(torch, a) for a in (Rh, Wh, Sh, Ph, Xh))
    cf, lv = dev(torch, coef), dev(torch, live)
    rr = torch.full((Rh.shape[1],), float("nan"), dtype=torch.float64, device="cuda")
    handle.mscg_update(cf, lv, R, W, S, P, X, rr=rr)
    return (R, W, S, P, X), cf, lv, rr


def check_mscg(lz, handle, torch, n, b, dtype, s=3, seed=0, live=None):
    host = mscg_inputs(n, b, dtype, s, seed, live)
    (Rh, Wh, Sh, Ph, Xh), coef, live, zc, ac, fc = host
    (R, W, S, P, X), cf, lv, rr = run_mscg(handle, torch, host)
    eps, what = EPS[dtype], f"n={n} b={b} {dtype.__name__} s={s}"
    rnd = lambda v: f64(np.asarray(v).astype(dtype))
    al, be = rnd(coef[:b]), rnd(coef[b:2 * b])
    r, w = f64(Rh), f64(Wh)
    sv = np.where(be == 0, 0.0, f64(Sh))
    s1 = be * sv + w
    r1 = -al * s1 + r
    dS = 3 * eps * (np.abs(be * sv) + np.abs(w))
    dR = 3 * eps * (np.abs(al * s1) + np.abs(r)) + np.abs(al) * dS
    got = {k: f64(t.cpu().numpy()) for k, t in (("S", S), ("R", R), ("P", P), ("X", X))}
    worst = 0.0
    checks = [("S", got["S"], s1, dS), ("R", got["R"], r1, dR)]
    for k in range(s):
        o = (2 + 3 * k) * b
        ze, ak, bk = rnd(coef[o:o + b]), rnd(coef[o + b:o + 2 * b]), rnd(coef[o + 2 * b:o + 3 * b])
        if not live[k]:
            assert same_bits(torch, P[k], dev(torch, Ph[k])) and same_bits(torch, X[k], dev(torch, Xh[k])), \
                f"{what}: shift {k} is not live: P_k and X_k bit for bit"
            continue
        run = ak != 0                                    # the columns the shift's step touches
        p = np.where(bk == 0, 0.0, f64(Ph[k]))[:, run]  # b_k == 0: P_k is not used
        x, rk = f64(Xh[k])[:, run], r[:, run]
        p1 = bk[run] * p + ze[run] * rk
        x1 = ak[run] * p1 + x
        dP = 3 * eps * (np.abs(bk[run] * p) + np.abs(ze[run] * rk))
        dX = 3 * eps * (np.abs(ak[run] * p1) + np.abs(x)) + np.abs(ak[run]) * dP
        checks += [(f"P_{k}", got["P"][k][:, run], p1, dP), (f"X_{k}", got["X"][k][:, run], x1, dX)]
        if ac[k] is not None:
            assert same_bits(torch, P[k][:, ac[k]], dev(torch, Ph[k][:, ac[k]])) \
                and same_bits(torch, X[k][:, ac[k]], dev(torch, Xh[k][:, ac[k]])), f"{what}: a_{k} = 0 keeps P_k and X_k"
        if fc[k] is not None:
            t = (coef[o + fc[k]].astype(dtype) * Rh[:, fc[k]]).astype(dtype)
            assert same_bits(torch, P[k][:, fc[k]], dev(torch, t)), f"{what}: b_{k} = 0 gives p' = t"
    for name, g, ref, bound in checks:
        assert np.isfinite(g).all(), f"{what}: NaN / Inf in {name}"
        err = np.abs(g - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max(initial=0.0)))  # (b = 1, a_k = 0: no column)
        assert (err <= bound).all(), f"{what}: {name}"
    assert torch.equal(W, dev(torch, Wh)) and torch.equal(cf, dev(torch, coef)) and torch.equal(lv, dev(torch, live)), \
        f"{what}: W, coef and live are read only"
    if zc is not None:
        assert torch.equal(R[:, zc], dev(torch, Rh[:, zc])), f"{what}: alpha = 0 leaves R bit for bit"
    rrh, sq = rr.cpu().numpy(), (got["R"] ** 2).sum(axis=0)
    assert np.isfinite(rrh).all(), f"{what}: NaN in rr"
    rerr = np.abs(rrh - sq)
    print(f"{what}: max err/bound {worst:.3f}; rr max err/bound {(rerr / ((n + 2) * EPS64 * sq)).max():.3e}")
    assert (rerr <= (n + 2) * EPS64 * sq).all(), f"{what}: rr"
    return R, S, P, X, rr


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_update_parity(lz, handle, torch_cuda, b, dtype):
    rpb, rows = update_rows(lz, b, dtype)
    assert math.ceil(rows[-1] / rpb) > lz.CG_GRID_CAP and math.ceil(rows[-2] / rpb) == 257
    for n in rows:
        check_mscg(lz, handle, torch_cuda, n, b, dtype, seed=n % 1000 + b)
    if b == 1:  # every kind of its one column
        for seed in (0, 1, 2):
            check_mscg(lz, handle, torch_cuda, rows[3], b, dtype, seed=seed)


@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
@pytest.mark.parametrize("live", [(1, 0, 1), (0, 1, 0), (0, 0, 0), (1, 1, 0, 1)])
def test_update_skips_a_shift_that_is_not_live(lz, handle, torch_cuda, b, dtype, live):
    """live[k] = 0 with non-zero coefficients: NaN-filled P_k and X_k keep every bit (check_mscg
    compares them); the live shifts and the seed's blocks are as ever."""
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3]):
        host = mscg_inputs(n, b, dtype, len(live), 11, live)
        for k, on in enumerate(live):
            if not on:
                host[0][3][k][:] = np.nan
                host[0][4][k][:] = np.nan
        (R, W, S, P, X), cf, lv, rr = run_mscg(handle, torch_cuda, host)
        for k, on in enumerate(live):
            if not on:
                assert same_bits(torch_cuda, P[k], dev(torch_cuda, host[0][3][k]))
                assert same_bits(torch_cuda, X[k], dev(torch_cuda, host[0][4][k]))
        assert torch_cuda.isfinite(R).all() and torch_cuda.isfinite(S).all() and torch_cuda.isfinite(rr).all()
        check_mscg(lz, handle, torch_cuda, n, b, dtype, s=len(live), seed=11, live=live)


@pytest.mark.parametrize("b,dtype", FORM128)
def test_update_forms_agree(lz, handle, torch_cuda, monkeypatch, b, dtype):
    """The 128-byte-row form and the generic form finish every element with the same operations:
    the same bits in R, S, P, X (rr sums in another order); plain loads and stores: every bit."""
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[4]):
        fast = check_mscg(lz, handle, torch_cuda, n, b, dtype, seed=7)
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_GENERIC", "1")
            gen = check_mscg(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for k, u, v in zip("RSPX", fast[:4], gen[:4]):
            assert same_bits(torch_cuda, u, v), f"n={n}: {k} differs between the forms"
        with monkeypatch.context() as mp:
            mp.setenv("LZ_CG_NT", "0")
            plain = check_mscg(lz, handle, torch_cuda, n, b, dtype, seed=7)
        for u, v in zip(fast, plain):
            assert same_bits(torch_cuda, u, v), "plain loads and stores: every bit, rr included"


@pytest.mark.parametrize("b,dtype", FORM128 + GENERIC)
def test_one_shift_is_cg_update(lz, handle, torch_cuda, b, dtype):
    """s = 1, coef = [alpha | beta | 1 | alpha | beta]: cg_update's bits in R, S, X, rr, and in P where
    alpha != 0 (cg_update also rewrites a frozen column's P)."""
    torch = torch_cuda
    rpb, rows = update_rows(lz, b, dtype)
    for n in (rows[0], rows[3], rows[-1]):
        (Rh, Wh, Ph, Sh, Xh), coef, zc, fc = update_inputs(n, b, dtype, seed=n % 1000 + b + 1)
        R, W, P, S, X = (dev(torch, a) for a in (Rh, Wh, Ph, Sh, Xh))
        rr = handle.cg_update(dev(torch, coef), R, W, P, S, X)
        R2, W2, P2, S2, X2 = (dev(torch, a) for a in (Rh, Wh, Ph[None], Sh, Xh[None]))
        cf = np.concatenate([coef, np.ones(b), coef])
        rr2 = handle.mscg_update(dev(torch, cf), dev(torch, np.ones(1, np.int32)), R2, W2, S2, P2, X2)
        for k, u, v in (("R", R, R2), ("S", S, S2), ("X", X, X2[0]), ("rr", rr, rr2)):
            assert same_bits(torch, u, v), f"n={n}: {k}"
        run = torch.from_numpy(coef[:b].astype(dtype) != 0).cuda()
        assert same_bits(torch, P[:, run], P2[0][:, run]), f"n={n}: P on the live columns"
        assert same_bits(torch, P2[0][:, ~run], dev(torch, Ph)[:, ~run])


def test_sixteen_shifts(lz, handle, torch_cuda):
    rpb, rows = update_rows(lz, 16, F64)
    live = [1] * 16
    live[5] = live[15] = 0
    for n in (rows[1], rows[4]):
        check_mscg(lz, handle, torch_cuda, n, 16, F64, s=16, seed=3)
        check_mscg(lz, handle, torch_cuda, n, 16, F64, s=16, seed=4, live=live)


def test_update_arguments(lz, handle, torch_cuda):
    torch = torch_cuda
    n, b, s = 40, 16, 2
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device="cuda")
    R, W, S, P, X = z(n, b), z(n, b), z(n, b), z(s, n, b), z(s, n, b)
    cf, lv = z((2 + 3 * s) * b), torch.ones(s, dtype=torch.int32, device="cuda")
    E = lz.LanczosError
    for args in [(R, R, S, P, X), (R, W, R, P, X), (R, W, S, P, P), (P[1], W, S, P, X), (R, W, X[0], P, X)]:
        with pytest.raises(E):
            handle.mscg_update(cf, lv, *args)
    with pytest.raises(E):
        handle.mscg_update(cf[:-1], lv, R, W, S, P, X)
    with pytest.raises(E):
        handle.mscg_update(cf, lv[:1], R, W, S, P, X)
    with pytest.raises(E):
        handle.mscg_update(cf, lv.double(), R, W, S, P, X)
    with pytest.raises(E):
        handle.mscg_update(z(2 * b), lv[:0], R, W, S, P[:0], X[:0])          # s = 0
    with pytest.raises(E):
        handle.mscg_update(z(53 * b), torch.ones(17, dtype=torch.int32, device="cuda"), R, W, S, z(17, n, b),
                           z(17, n, b))                                       # s = 17
    with pytest.raises(E):
        handle.mscg_update(z(8 * 65), lv, z(n, 65), z(n, 65), z(n, 65), z(s, n, 65), z(s, n, 65))
    handle.mscg_update(cf, lv, R, W, S, P, X)  # the call after the errors succeeds


# ------------------------------------------------------------ 2. solve_shifts
def residuals(A, D, Bh, Xk, sh, dtype):
    """The fp64 residual norms of one shift's X and the rounding of the dtype's own evaluation."""
    eps, B64 = EPS[dtype], f64(Bh)
    sgm = float(dtype(sh))
    r = np.linalg.norm(B64 - (D @ Xk + sgm * Xk), axis=0)
    nnz_row = np.diff(A.row_ptr)[:, None]
    rnd = np.linalg.norm((nnz_row + 3) * eps * (np.abs(D) @ np.abs(Xk) + abs(sgm) * np.abs(Xk) + np.abs(B64)), axis=0)
    return r, rnd


@pytest.mark.parametrize("grid,b,dtype,name", CASES)
def test_solve_shifts(lz, handle, torch_cuda, grid, b, dtype, name):
    torch = torch_cuda
    A, D, _ = operator(lz, grid, dtype)
    shifts, tol, n = SHIFT_LISTS[name], TOL[dtype], A.n
    Bh = rhs(n, b, dtype)
    B = dev(torch, Bh)
    out = handle.solve_shifts(lz.CsrDevice.from_host(A), B, shifts)
    assert torch.equal(B, dev(torch, Bh)), "B is read only"
    ref = restated(lz, grid, b, dtype, name)
    s = len(shifts)
    assert out["X"].shape == (s, n, b) and out["seed"] == int(np.argmin(shifts)) == ref["seed"]
    Xh = f64(out["X"].cpu().numpy())
    assert np.isfinite(Xh).all()
    bn = np.linalg.norm(f64(Bh), axis=0)
    worst = 0.0
    for k, sh in enumerate(shifts):
        r, rnd = residuals(A, D, Bh, Xh[k], sh, dtype)
        worst = max(worst, float((r / np.maximum(tol * bn, 1e-300)).max()))
        assert (r <= tol * bn + rnd).all(), f"shift {sh}: the fp64 residual of the returned X"
        assert (np.abs(out["resid"][k] * bn - r) <= rnd + (n + 2) * EPS64 * r).all(), f"shift {sh}: resid"
    print(f"{grid} b={b} {dtype.__name__} {name}: iterations {out['iterations']} (restated {ref['iterations']}), per "
          f"shift {out['iters'].max(axis=1).tolist()} (restated {ref['iters'].max(axis=1).tolist()}), n_spmm "
          f"{out['n_spmm']}, polished pairs {out['finished']} of {s * b}, finish iters {int(out['finish_iters'].sum())}, "
          f"restarts {out['restarts']}, max true |r| / (tol |b|) {worst:.3f}, max est / tol {(out['est'] / tol).max():.3f}")
    assert (out["status"] == MET).all() and out["converged"].all(), f"status {out['status']}"
    assert (out["iters"] <= np.ceil(1.1 * ref["iters"]) + 2).all(), "iterations against the restatement"
    finishing_cap(out)
    assert out["finished"] == int((out["finish_iters"] > 0).sum())
    if out["finished"] == 0:
        assert out["n_spmm"] == out["iterations"] + s and out["restarts"] == 0
    else:  # a polished shift: its iterations in chunks, and one more measurement at the least
        extra = sum(int(f.max()) + 1 for f in out["finish_iters"] if f.max() > 0)
        assert out["n_spmm"] >= out["iterations"] + s + extra
    assert out["iterations"] >= out["iters"].max() and (out["est"] <= tol).all()


@pytest.fixture(scope="module")
def lap(lz, handle, torch_cuda):
    """The 40 x 36 Laplacian at fp64, b = 16, the unordered shifts: one solve."""
    class P:
        pass
    s = P()
    s.A, s.D, _ = operator(lz, (40, 36), F64)
    s.Ad = lz.CsrDevice.from_host(s.A)
    s.Bh = rhs(s.A.n, 16, F64)
    s.B = dev(torch_cuda, s.Bh)
    s.shifts = SHIFT_LISTS["unordered"]
    s.out = handle.solve_shifts(s.Ad, s.B, s.shifts)
    assert s.out["converged"].all()
    return s


@pytest.mark.parametrize("b,dtype", FORM128 + [(5, F64)])
@pytest.mark.parametrize("shift", [0.5, 0.0])
def test_one_shift_is_solve(lz, handle, torch_cuda, b, dtype, shift):
    torch = torch_cuda
    A = operator(lz, (40, 36), dtype)[0]
    Ad, B = lz.CsrDevice.from_host(A), dev(torch, rhs(A.n, b, dtype))
    one, plain = handle.solve_shifts(Ad, B, [shift]), handle.solve(Ad, B, shift=shift)
    assert plain["converged"].all()
    assert same_bits(torch, one["X"][0], plain["X"]), "X bit for bit"
    assert np.array_equal(one["iters"][0] + one["finish_iters"][0], plain["iters"])
    assert np.array_equal(one["status"][0], plain["status"]) and np.array_equal(one["resid"][0], plain["resid"])
    assert one["seed"] == 0 and one["n_spmm"] == plain["n_spmm"] - 1  # (no SpMM measures the zero start)


def test_permuted_shifts(lz, lap, handle, torch_cuda):
    perm = [2, 0, 3, 1]
    o = handle.solve_shifts(lap.Ad, lap.B, [lap.shifts[i] for i in perm])
    assert o["seed"] == perm.index(lap.out["seed"])
    for j, i in enumerate(perm):
        assert same_bits(torch_cuda, o["X"][j], lap.out["X"][i]), f"shift {lap.shifts[i]}"
        assert np.array_equal(o["iters"][j], lap.out["iters"][i]) and np.array_equal(o["resid"][j], lap.out["resid"][i])
    assert o["iterations"] == lap.out["iterations"] and o["n_spmm"] == lap.out["n_spmm"]


def test_zero_and_nan_columns(lz, lap, handle, torch_cuda):
    """As in solve: a zero column is met at once (X = 0, resid = est = 0, no iterations); a NaN
    column ends with status 2 at the first step, its X untouched; the other columns do not notice."""
    Bh = lap.Bh.copy()
    Bh[:, 7] = np.nan
    o = handle.solve_shifts(lap.Ad, dev(torch_cuda, Bh), lap.shifts)
    ok = np.arange(16) != 7
    assert (o["status"][:, ok] == MET).all() and (o["status"][:, 7] == NOT_PD).all()
    assert (o["iters"][:, [3, 7]] == 0).all() and (o["finish_iters"][:, [3, 7]] == 0).all()
    assert (o["X"][:, :, [3, 7]] == 0).all() and (o["resid"][:, 3] == 0).all() and (o["est"][:, 3] == 0).all()
    assert same_bits(torch_cuda, o["X"][:, :, ok], lap.out["X"][:, :, ok])
    assert np.array_equal(o["iters"][:, ok], lap.out["iters"][:, ok])
    for k, sh in enumerate(lap.shifts[:2]):
        p = handle.solve(lap.Ad, dev(torch_cuda, Bh), shift=sh)
        assert np.array_equal(p["status"], o["status"][k]) and (p["iters"][[3, 7]] == 0).all()


def test_indefinite_seed(lz, lap, handle, torch_cuda):
    """Shifts [-0.5, 0, 1]: A - 0.5 I is indefinite, so the seed's columns break down (status 2 at
    -0.5); the finishing phase solves the two shifts whose operator is positive definite."""
    shifts = [-0.5, 0.0, 1.0]
    o = handle.solve_shifts(lap.Ad, lap.B, shifts)
    nz = np.arange(16) != 3
    print(f"indefinite seed: shared iters {o['iters'].max(axis=1).tolist()}, finish iters "
          f"{o['finish_iters'].max(axis=1).tolist()}, n_spmm {o['n_spmm']}")
    assert (o["status"][0, nz] == NOT_PD).all() and (o["status"][1:] == MET).all() and o["status"][0, 3] == MET
    assert torch_cuda.isfinite(o["X"][1:]).all()
    bn = np.linalg.norm(lap.Bh, axis=0)
    for k in (1, 2):
        r, rnd = residuals(lap.A, lap.D, lap.Bh, f64(o["X"][k].cpu().numpy()), shifts[k], F64)
        assert (r <= 1e-10 * bn + rnd).all()


def test_max_iter(lz, lap, handle, torch_cuda):
    o = handle.solve_shifts(lap.Ad, lap.B, lap.shifts, max_iter=5)
    nz = np.arange(16) != 3
    assert (o["status"][:, nz] == SPENT).all() and (o["iters"][:, nz] == 5).all() and (o["finish_iters"] == 0).all()
    assert (o["status"][:, 3] == MET).all() and o["restarts"] == 0 and torch_cuda.isfinite(o["X"]).all()
    assert o["n_spmm"] == o["iterations"] + len(lap.shifts)


def test_check_every(lz, lap, handle, torch_cuda):
    o1, o7 = (handle.solve_shifts(lap.Ad, lap.B, lap.shifts, check_every=k) for k in (1, 7))
    for o in (o1, o7):
        assert same_bits(torch_cuda, o["X"], lap.out["X"]) and np.array_equal(o["iters"], lap.out["iters"])
    assert o1["iterations"] <= o7["iterations"] < o1["iterations"] + 7


def test_same_bits_after_an_unrelated_solve(lz, lap, handle, torch_cuda):
    A2 = lz.gen_banded(1000, nnz_per_row=9, halfwidth=32, seed=3, dtype=F32)
    B2 = dev(torch_cuda, rhs(A2.n, 8, F32))
    handle.solve(lz.CsrDevice.from_host(A2), B2, shift=1.0 - lz.gershgorin(A2)[0])
    handle.solve_shifts(lz.CsrDevice.from_host(A2), B2, [3.0 - lz.gershgorin(A2)[0], 2.0 - lz.gershgorin(A2)[0]])
    again = handle.solve_shifts(lap.Ad, lap.B, lap.shifts)
    assert same_bits(torch_cuda, again["X"], lap.out["X"])
    for k in ("iters", "finish_iters", "status", "resid", "est"):
        assert np.array_equal(again[k], lap.out[k]), k
    assert again["n_spmm"] == lap.out["n_spmm"]


def test_arguments(lz, lap, handle, torch_cuda):
    torch = torch_cuda
    E = lz.LanczosError
    n, b = lap.A.n, 16
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, [])                                   # s = 0
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, list(range(17)))                      # s = 17
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, torch.zeros(n, 65, dtype=torch.float64, device="cuda"), [0.0, 1.0])
    buf = torch.zeros(8 * n * b, dtype=torch.float64, device="cuda")
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, [0.0, 1.0], work=buf[:4 * n * b])     # work too short: 3 + s blocks
    with pytest.raises(E):                                                       # work holds B
        handle.solve_shifts(lap.Ad, buf[n * b:2 * n * b].view(n, b), [0.0, 1.0], work=buf[:5 * n * b])
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, [0.0, float("nan")])
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, [0.0, float("inf")])
    with pytest.raises(E):
        handle.solve_shifts(lap.Ad, lap.B, [0.0], tol=0.0)
    with pytest.raises(E):
        handle.solve_shifts(lz.CsrDevice.from_host(lap.A, n_cols=n + 1), lap.B, [0.0])
    assert b"argument error" in handle.L.lz_last_error()
    o = handle.solve_shifts(lap.Ad, lap.B, lap.shifts, work=buf[:7 * n * b])     # the call after the errors succeeds
    assert same_bits(torch, o["X"], lap.out["X"])
