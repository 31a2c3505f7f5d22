"""Kernel polynomial method, host side, without a GPU: lzh_kpm_moments, lzh_jackson,
lzh_kpm_count and lzh_kpm_density against NumPy restatements written here; the statistical
condition the GPU tests rest on, checked on fixed probes; and Handle.spectral_moments /
KpmMoments on a stand-in Handle that opens no device (cheb_moments is the NumPy recurrence).

The operator is gen_laplace2d(40, 36) with the bounds (-0.08, 8.08); its exact trace moments
sum_i cos(k acos((lambda_i - c0) / e)) come from numpy.linalg.eigvalsh.
"""
import ctypes

import numpy as np
import pytest

LO, HI = -0.08, 8.08
M = 129                      # moments, K = 64 steps
INTERVALS = [(0.0, 0.5), (0.0, 1.0), (3.0, 5.0), (7.0, 8.0), (1.95, 2.05)]
PROBES = 64
# The probe seed: the first of 0, 1, 2, ... whose restated estimate lies within 2 stderr of the
# exact-moment count at all five intervals: seed 0, at 1.50, 0.34, 0.95, 0.98 and 0.71 stderr
# (of seeds 0 .. 11, only 2 and 10 miss 2 stderr; test_statistical_condition prints the ratios).
PROBE_SEED = 0


def dense(A):
    D = np.zeros((A.n, A.n))
    for r in range(A.n):
        s = slice(A.row_ptr[r], A.row_ptr[r + 1])
        D[r, A.col[s]] = A.val[s]
    return D


def probes_pm1(n, seed=PROBE_SEED, cols=PROBES):
    """The fixed +-1 probes of the CPU and the GPU end-to-end tests."""
    return np.random.default_rng(seed).integers(0, 2, (n, cols)).astype(np.float64) * 2.0 - 1.0


def raw_dots(mul, X0, K, lo=LO, hi=HI, dtype=np.float64, coef=None):
    """lz_cheb_moments restated: (K+1, 2, b) dots of t_0 = X0, t_1 = Ah t_0, t_{k+1} = 2 Ah t_k -
    t_{k-1}, each step a (A t) + c t + d t_prev in `dtype` with the coefficients rounded to
    `coef` (default dtype), the dots in fp64 (longdouble when dtype is)."""
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    acc = np.longdouble if dtype == np.longdouble else np.float64
    cf = lambda v: dtype((coef or dtype)(v))
    t0 = X0.astype(dtype)
    dots = np.zeros((K + 1, 2, X0.shape[1]), acc)
    dots[0, 0] = (t0.astype(acc) ** 2).sum(axis=0)
    prev, cur = None, t0
    for k in range(1, K + 1):
        if k == 1:
            nxt = cf(1.0 / e) * mul(cur) + cf(-c0 / e) * cur
        else:
            nxt = cf(2.0 / e) * mul(cur) + (cf(-2.0 * c0 / e) * cur + cf(-1.0) * prev)
        nxt = nxt.astype(dtype)
        dots[k, 0] = (nxt.astype(acc) ** 2).sum(axis=0)
        dots[k, 1] = (nxt.astype(acc) * cur.astype(acc)).sum(axis=0)
        prev, cur = cur, nxt
    return dots


def moments_restated(dots):
    """The doubling identities: (K+1, 2, b) -> (2K+1, b)."""
    K = dots.shape[0] - 1
    mu = np.empty((2 * K + 1, dots.shape[2]), dots.dtype)
    mu[0], mu[1] = dots[0, 0], dots[1, 1]
    for k in range(1, K + 1):
        mu[2 * k] = 2 * dots[k, 0] - mu[0]
        if k >= 2:
            mu[2 * k - 1] = 2 * dots[k, 1] - mu[1]
    return mu


def jackson_restated(m):
    k = np.arange(m)
    q = np.pi / (m + 1)
    return ((m + 1 - k) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (m + 1)


def gamma(m, a, b, lo=LO, hi=HI):
    """The Chebyshev coefficients of the indicator of [a, b]."""
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    ta, tb = (np.arccos(np.clip((x - c0) / e, -1.0, 1.0)) for x in (a, b))
    k = np.arange(1, m)
    return np.concatenate([[(ta - tb) / np.pi], 2.0 * (np.sin(k * ta) - np.sin(k * tb)) / (k * np.pi)])


def count_restated(mu, g, a, b, lo=LO, hi=HI):
    """sum_k g_k gamma_k mu_k for mu (M,) or (M, probes)."""
    w = gamma(mu.shape[0], a, b, lo, hi) * (1.0 if g is None else g)
    return w @ mu


def density_restated(mu, g, x, lo=LO, hi=HI):
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    xh = (np.asarray(x, float) - c0) / e
    inside = (xh > -1) & (xh < 1)
    th = np.arccos(np.clip(xh, -1, 1))
    k = np.arange(mu.shape[0])
    w = (1.0 if g is None else g) * np.where(k == 0, 1.0, 2.0)
    s = np.cos(np.outer(th, k)) @ (w[:, None] * mu.reshape(mu.shape[0], -1))
    rho = s / (np.pi * e * np.sqrt(np.where(inside, 1 - xh * xh, 1.0)))[:, None]
    rho = np.where(inside[:, None], rho, 0.0)
    return rho[:, 0] if mu.ndim == 1 else rho


def exact_moments(ev, m, lo=LO, hi=HI):
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    return np.cos(np.outer(np.arange(m), np.arccos((ev - c0) / e))).sum(axis=1)


@pytest.fixture(scope="module")
def lap(lz):
    class P:
        pass
    s = P()
    s.A = lz.gen_laplace2d(40, 36)
    s.D = dense(s.A)
    s.ev = np.linalg.eigvalsh(s.D)
    s.n = s.A.n
    s.exact = exact_moments(s.ev, M)
    return s


# ------------------------------------------------------ identities, coefficients
@pytest.mark.parametrize("K,b", [(1, 1), (2, 3), (7, 5), (64, 16)])
def test_doubling_identities(lz, lap, K, b):
    """lzh_kpm_moments equals its restatement, and the doubled moments equal the direct
    x^T T_k x within 64 (2K+1) eps max|mu|."""
    X = probes_pm1(lap.n, seed=5, cols=b)
    dots = raw_dots(lambda t: lap.D @ t, X, K)
    mu = lz.kpm_moments(dots)
    assert mu.shape == (2 * K + 1, b)
    assert np.array_equal(mu, moments_restated(dots))
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    Ah = (lap.D - c0 * np.eye(lap.n)) / e
    T = [X, Ah @ X]
    for _ in range(2, 2 * K + 1):
        T.append(2 * Ah @ T[-1] - T[-2])
    direct = np.array([(X * t).sum(axis=0) for t in T])
    bound = 64 * (2 * K + 1) * np.finfo(float).eps * np.abs(direct).max()
    print(f"K={K} b={b}: max|doubled - direct| {np.abs(mu - direct).max():.3e}, bound {bound:.3e}")
    assert np.abs(mu - direct).max() <= bound


def test_jackson(lz):
    for m in (1, 2, 17, 129, 1000):
        g = lz.jackson(m)
        assert g.shape == (m,) and abs(g[0] - 1.0) <= 1e-15
        assert np.abs(g - jackson_restated(m)).max() <= 1e-14
        assert (np.diff(g) < 0).all() and (g > 0).all()
        if m >= 17:  # the last factor is O(1 / M^2)
            assert g[-1] <= 20.0 / m ** 2


def test_count_exact_moments(lz, lap):
    """On exact trace moments: the restated formula to 1e-10 n for any interval; the true count
    within 0.5 for an interval whose ends sit in gaps wider than 2 pi e / M."""
    g = lz.jackson(M)
    for damping, gg in (("jackson", g), (None, None)):
        for a, b in INTERVALS + [(-1.0, 9.0), (2.0, 2.0), (-5.0, 0.3), (7.9, 20.0)]:
            got = lz.kpm_count(lap.exact, LO, HI, a, b, damping)
            assert abs(got - count_restated(lap.exact, gg, a, b)) <= 1e-10 * lap.n
    assert abs(lz.kpm_count(lap.exact, LO, HI, LO, HI) - lap.n) <= 1e-9 * lap.n
    # gaps: the Laplacian's 1440 eigenvalues leave no gap of 2 pi e / 129 = 0.2, so take the two
    # widest gaps and as many moments as make them 2.5 x 2 pi e / M wide
    gaps = np.diff(lap.ev)
    i, j = np.sort(np.argsort(gaps)[-2:])
    m2 = int(np.ceil(2.5 * 2 * np.pi * (0.5 * (HI - LO)) / gaps[[i, j]].min()))
    width = 2 * np.pi * (0.5 * (HI - LO)) / m2
    assert m2 <= 20000 and min(gaps[i], gaps[j]) > 2 * width
    ex2 = exact_moments(lap.ev, m2)
    a, b = 0.5 * (lap.ev[i] + lap.ev[i + 1]), 0.5 * (lap.ev[j] + lap.ev[j + 1])
    got = lz.kpm_count(ex2, LO, HI, a, b)
    print(f"gaps after eigenvalues {i}, {j} ({gaps[i]:.4f}, {gaps[j]:.4f}; 2 pi e / M = {width:.4f}): "
          f"count {got:.4f}, true {j - i}")
    assert abs(got - (j - i)) <= 0.5


def test_density(lz, lap):
    g = lz.jackson(M)
    x = np.concatenate([np.linspace(-1.0, 9.0, 41), [LO, HI]])
    for damping, gg in (("jackson", g), (None, None)):
        rho = lz.kpm_density(lap.exact, LO, HI, x, damping)
        ref = density_restated(lap.exact, gg, x)
        assert np.abs(rho - ref).max() <= 1e-10 * lap.n
        assert (rho[(x <= LO) | (x >= HI)] == 0).all()
    # Gauss-Chebyshev quadrature of rho over (lo, hi): exact for the series, so the integral
    # is g_0 mu_0 = n up to rounding
    q = 400
    th = (np.arange(q) + 0.5) * np.pi / q
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    rho = lz.kpm_density(lap.exact, LO, HI, c0 + e * np.cos(th))
    total = (np.pi / q) * (rho * e * np.sin(th)).sum()
    assert abs(total - lap.n) <= 1e-9 * lap.n
    assert (rho > -1e-9).all(), "the Jackson kernel is positive"


def test_argument_errors(lz, lap):
    L = lz.host_lib()
    out, mu = np.empty(1), lap.exact
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.lzh_kpm_moments(0, 4, p(mu), p(mu)) == -1 and L.lzh_kpm_moments(2, 0, p(mu), p(mu)) == -1
    assert L.lzh_kpm_moments(2, 4, None, p(mu)) == -1
    assert L.lzh_jackson(0, p(out)) == -1 and L.lzh_jackson(4, None) == -1
    assert L.lzh_kpm_count(0, p(mu), None, LO, HI, 0.0, 1.0, p(out)) == -1
    assert L.lzh_kpm_count(M, p(mu), None, HI, LO, 0.0, 1.0, p(out)) == -1
    assert L.lzh_kpm_count(M, p(mu), None, LO, float("inf"), 0.0, 1.0, p(out)) == -1
    assert L.lzh_kpm_count(M, p(mu), None, LO, HI, 1.0, 0.0, p(out)) == -1
    assert L.lzh_kpm_count(M, None, None, LO, HI, 0.0, 1.0, p(out)) == -1
    assert L.lzh_kpm_density(M, p(mu), None, LO, LO, 1, p(out), p(out)) == -1
    assert L.lzh_kpm_density(M, p(mu), None, LO, HI, -1, p(out), p(out)) == -1
    assert L.lzh_kpm_density(M, p(mu), None, LO, HI, 1, None, p(out)) == -1
    assert L.lzh_kpm_count(M, p(mu), None, LO, HI, 0.0, 1.0, p(out)) == 0
    for bad in (lambda: lz.kpm_moments(np.zeros((3, 3, 2))), lambda: lz.jackson(0),
                lambda: lz.kpm_count(mu, HI, LO, 0.0, 1.0), lambda: lz.kpm_count(mu, LO, HI, 0.0, 1.0, "lorentz"),
                lambda: lz.kpm_density(mu, LO, LO, [1.0])):
        with pytest.raises(lz.LanczosError):
            bad()


# ------------------------------------------------------ the statistical condition
def probe_counts(lap, mu):
    """Per interval: (estimate, stderr, exact-moment count) with Jackson damping."""
    g = jackson_restated(M)
    out = []
    for a, b in INTERVALS:
        per = count_restated(mu, g, a, b)
        out.append((per.mean(), per.std(ddof=1) / np.sqrt(per.size), count_restated(lap.exact, g, a, b)))
    return out


def test_statistical_condition(lz, lap):
    """64 fixed +-1 probes, M = 129: the restated estimate lies within 3 stderr of the
    exact-moment count (same damping) at every interval; PROBE_SEED was chosen so that it
    holds within 2, which leaves the GPU tests, on the same probes, a full stderr of room."""
    X = probes_pm1(lap.n)
    mu = moments_restated(raw_dots(lambda t: lap.D @ t, X, (M - 1) // 2))
    ratios = []
    for (a, b), (est, se, ref) in zip(INTERVALS, probe_counts(lap, mu)):
        true = int(((lap.ev >= a) & (lap.ev <= b)).sum())
        ratios.append(abs(est - ref) / se)
        print(f"[{a}, {b}]: estimate {est:.2f} +- {se:.2f}, exact moments {ref:.2f} (true count {true}): "
              f"{ratios[-1]:.2f} stderr")
    print(f"seed {PROBE_SEED}: ratios " + " ".join(f"{r:.2f}" for r in ratios))
    assert max(ratios) <= 3.0
    assert max(ratios) <= 2.0, "PROBE_SEED no longer meets the 2 stderr it was chosen for"


# ------------------------------------------------------ the driver, no device
def make_standin(lz):
    import torch
    from test_restart_driver import make_standin as restart_standin
    _, DenseCsr = restart_standin(lz)

    class KpmHandle(lz.Handle):
        """No device: cheb_moments is raw_dots on the dense operator; calls are recorded."""

        def __init__(self, blow_up=False):
            self._h, self.calls, self.blow_up = None, [], blow_up

        def close(self):
            pass

        def cheb_moments(self, A, X0, K, lo, hi, work=None, dots=None):
            self.calls.append((K, lo, hi, tuple(X0.shape), X0.numpy().copy()))
            assert work.numel() == 3 * A.n * X0.shape[1] and tuple(dots.shape) == (K + 1, 2, X0.shape[1])
            d = raw_dots(lambda t: A.dense @ t, X0.numpy(), K, lo, hi)
            if self.blow_up:
                d[-1, 0, 0] = np.inf
            dots.copy_(torch.from_numpy(d))
            return dots

    return KpmHandle, DenseCsr


def test_driver(lz, lap):
    import torch
    KpmHandle, DenseCsr = make_standin(lz)
    A = DenseCsr(lap.n, lap.n, lap.A.row_ptr, lap.A.col, lap.A.val)
    X = probes_pm1(lap.n, cols=8)
    h = KpmHandle()
    km = h.spectral_moments(A, n_moments=20, b=4, bounds=(0.0, 8.0), pad=0.01, X0=torch.from_numpy(X))
    # K = ceil(19 / 2) = 10, two blocks, the bounds moved out by pad x width
    assert [(c[0], c[3]) for c in h.calls] == [(10, (lap.n, 4))] * 2
    assert all(abs(c[1] - LO) <= 1e-15 and abs(c[2] - HI) <= 1e-15 for c in h.calls)
    assert np.array_equal(h.calls[0][4], X[:, :4]) and np.array_equal(h.calls[1][4], X[:, 4:])
    assert (km.n, km.n_spmm, km.mu.shape) == (lap.n, 20, (21, 8)) and abs(km.lo - LO) + abs(km.hi - HI) <= 1e-15
    # two blocks of 4 = one block of 8
    h8 = KpmHandle()
    km8 = h8.spectral_moments(A, n_moments=21, b=8, bounds=(0.0, 8.0), X0=torch.from_numpy(X))
    assert len(h8.calls) == 1 and km8.n_spmm == 10
    assert np.array_equal(km.mu, km8.mu)
    assert np.array_equal(km.mu, moments_restated(raw_dots(lambda t: lap.D @ t, X, 10)))
    # count / density: the mean of the per-probe values and their standard error
    g = jackson_restated(21)
    est, se = km.count(3.0, 5.0)
    per = count_restated(km.mu, g, 3.0, 5.0)
    assert abs(est - per.mean()) <= 1e-10 * lap.n and abs(se - per.std(ddof=1) / np.sqrt(8)) <= 1e-10 * lap.n
    est0, _ = km.count(3.0, 5.0, damping=None)
    assert abs(est0 - count_restated(km.mu, None, 3.0, 5.0).mean()) <= 1e-10 * lap.n
    x = np.linspace(-1, 9, 23)
    rho, rse = km.density(x)
    ref = density_restated(km.mu, g, x)
    assert rho.shape == rse.shape == (23,)
    assert np.abs(rho - ref.mean(axis=1)).max() <= 1e-10 * lap.n
    assert np.abs(rse - ref.std(axis=1, ddof=1) / np.sqrt(8)).max() <= 1e-10 * lap.n
    # default bounds: Gershgorin, [0, 8] for this operator; default probes: one block of b, drawn +-1
    hd = KpmHandle()
    kd = hd.spectral_moments(A, n_moments=5, b=4, seed=3)
    assert len(hd.calls) == 1 and hd.calls[0][0] == 2 and abs(kd.lo - LO) + abs(kd.hi - HI) <= 1e-12
    assert set(np.unique(hd.calls[0][4])) == {-1.0, 1.0}
    hd2 = KpmHandle()
    hd2.spectral_moments(A, n_moments=5, b=4, seed=3, probes=8)
    assert len(hd2.calls) == 2 and np.array_equal(hd2.calls[0][4], hd.calls[0][4])
    assert not np.array_equal(hd2.calls[1][4], hd2.calls[0][4])
    # eigcount
    he = KpmHandle()
    assert he.eigcount(A, 3.0, 5.0, n_moments=20, b=4, bounds=(0.0, 8.0), X0=torch.from_numpy(X)) == (est, se)


def test_driver_errors(lz, lap):
    import torch
    KpmHandle, DenseCsr = make_standin(lz)
    A = DenseCsr(lap.n, lap.n, lap.A.row_ptr, lap.A.col, lap.A.val)
    X = torch.from_numpy(probes_pm1(lap.n, cols=4))
    with pytest.raises(lz.LanczosError, match="bounds"):
        KpmHandle(blow_up=True).spectral_moments(A, n_moments=9, b=4, X0=X)
    for kw in (dict(probes=6), dict(n_moments=1), dict(bounds=(8.0, 0.0)), dict(bounds=(0.0, float("nan")))):
        with pytest.raises(lz.LanczosError):
            KpmHandle().spectral_moments(A, **{**dict(n_moments=9, b=4), **kw})
