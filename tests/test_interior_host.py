"""Interior eigenpairs, the parts that need no GPU: the window's Chebyshev coefficients
(lzh_cheb_window / cheb_window) against their closed form, against the Chebyshev projection of
the indicator by Gauss-Chebyshev quadrature and against kpm_count's weights; the new ABI
symbols and the argument errors they report without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = -0.08, 8.08


def closed_form(M, lo, hi, a, b, g):
    e, c0 = 0.5 * (hi - lo), 0.5 * (hi + lo)
    ta, tb = (np.arccos(np.clip((x - c0) / e, -1.0, 1.0)) for x in (a, b))
    k = np.arange(1, M)
    gam = np.concatenate([[(ta - tb) / np.pi], 2 * (np.sin(k * ta) - np.sin(k * tb)) / (k * np.pi)])
    return gam * (1.0 if g is None else g)


@pytest.mark.parametrize("damping", [None, "jackson"])
@pytest.mark.parametrize("degree", [0, 1, 2, 9, 100, 1000])
def test_cheb_window_closed_form(lz, degree, damping):
    M = degree + 1
    g = lz.jackson(M) if damping else None
    for a, b in [(3.0, 3.2), (LO, 1.0), (7.5, HI), (4.0, 4.0), (LO, HI)]:
        gam = lz.cheb_window(degree, LO, HI, a, b, damping=damping)
        assert gam.shape == (M,)
        ref = closed_form(M, LO, HI, a, b, g)
        # sin(k theta) with k theta up to 1000 pi: the argument's rounding, k theta eps, on a weight 2 / (k pi)
        assert np.abs(gam - ref).max() <= 16 * np.finfo(float).eps * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("degree", [1, 9, 100])
def test_cheb_window_is_the_projection_of_the_indicator(lz, degree):
    """gamma_k = (2 - [k == 0]) / pi * int_{theta_b}^{theta_a} cos(k theta) d theta: the
    Chebyshev projection of the indicator, here by the midpoint rule in theta (the
    Gauss-Chebyshev nodes) with N nodes.  A node interval cut by a window edge is the
    quadrature's error: at most 2 of them, each 2 pi / N wide at weight <= 2 / pi."""
    a, b, N = 3.0, 3.2, 2_000_000
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    th = (np.arange(N) + 0.5) * np.pi / N
    x = c0 + e * np.cos(th)
    ind = ((x >= a) & (x <= b)).astype(float)
    k = np.arange(degree + 1)
    proj = np.array([(1.0 if kk == 0 else 2.0) / N * (ind * np.cos(kk * th)).sum() for kk in k])
    gam = lz.cheb_window(degree, LO, HI, a, b, damping=None)
    assert np.abs(gam - proj).max() <= 2 * 2.0 / N + 1e-12
    # the damped coefficients are the undamped ones times the Jackson factors of the same length
    damped = gam * lz.jackson(degree + 1)
    assert np.abs(lz.cheb_window(degree, LO, HI, a, b) - damped).max() <= 4 * np.finfo(float).eps * np.abs(damped).max()


@pytest.mark.parametrize("damping", [None, "jackson"])
@pytest.mark.parametrize("M", [1, 2, 17, 513])
def test_cheb_window_matches_kpm_count(lz, M, damping):
    rng = np.random.default_rng(M)
    mu = rng.uniform(-1, 1, M) * 1000.0
    for a, b in [(3.0, 3.2), (0.5, 7.0), (LO, HI)]:
        gam = lz.cheb_window(M - 1, LO, HI, a, b, damping=damping)
        cnt = lz.kpm_count(mu, LO, HI, a, b, damping=damping)
        assert abs(cnt - gam @ mu) <= 1e-12 * (np.abs(gam) * np.abs(mu)).sum()


def test_cheb_window_series_approximates_the_indicator(lz):
    """The damped series is within a few per cent of 1 well inside the window and of 0 well
    outside (3 pi e / degree, three widths of the Jackson kernel, away from the edges), and
    never leaves [0, 1] by much."""
    degree, a, b = 400, 3.0, 4.0
    e, c0 = 0.5 * (HI - LO), 0.5 * (HI + LO)
    gam = lz.cheb_window(degree, LO, HI, a, b)
    x = np.linspace(LO, HI, 4001)
    p = np.cos(np.outer(np.arccos((x - c0) / e), np.arange(degree + 1))) @ gam
    res = 3 * np.pi * e / degree
    assert p.min() >= -1e-3 and p.max() <= 1 + 1e-3  # Jackson: no Gibbs overshoot
    assert (p[(x > a + res) & (x < b - res)] >= 0.98).all()
    assert (p[(x < a - res) | (x > b + res)] <= 0.02).all()


def test_cheb_window_arguments(lz):
    for bad in [(4, 8.0, 1.0, 3.0, 4.0), (4, 1.0, 1.0, 1.0, 1.0), (4, LO, HI, 3.2, 3.0), (4, LO, HI, -1.0, 3.0),
                (4, LO, HI, 3.0, 9.0), (4, LO, float("inf"), 3.0, 4.0), (-1, LO, HI, 3.0, 4.0)]:
        with pytest.raises(lz.LanczosError):
            lz.cheb_window(*bad)
    with pytest.raises(lz.LanczosError):
        lz.cheb_window(4, LO, HI, 3.0, 4.0, damping="lorentz")
    H = lz.host_lib()
    out = np.empty(4)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    assert H.lzh_cheb_window(0, LO, HI, 3.0, 4.0, None, p(out)) == -1   # M >= 1
    assert H.lzh_cheb_window(4, LO, HI, 3.0, 4.0, None, None) == -1      # gamma NULL
    assert H.lzh_cheb_window(4, LO, HI, 3.0, 4.0, None, p(out)) == 0


NEW = ["lz_csr_spmm_axpby4", "lz_cheb_series_apply", "lz_block_lanczos_reorth_series",
       "lz_block_lanczos_reorth_resume_series"]


def test_new_entry_points(lz):
    txt = open(os.path.join(ROOT, "include", "lz_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lz_\w+)\s*\(", body))
    out = subprocess.run(["nm", "-D", "--defined-only", lz.HIP_LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    bound = {n for n, _, _ in lz.HIP_SYMBOLS}
    L = lz.hip_lib()
    for name in NEW:
        assert name in declared and name in exported and name in bound and hasattr(L, name), name
    assert lz.LZ_K_AX4 == int(re.search(r"LZ_K_AX4\s*=\s*(0x[0-9a-fA-F]+)", body).group(1), 16)
    assert lz.LZ_K_AX4 & (lz.LZ_K_WIN | lz.LZ_K_YCM | lz.LZ_K_EPI | lz.LZ_K_AX3 | lz.LZ_K_DOT | 0xff) == 0


def test_new_entry_points_without_a_handle(lz):
    """No device: a NULL handle is reported (LZ_E_STATE, with a message), never dereferenced."""
    L = lz.hip_lib()
    g = (ctypes.c_double * 3)(0.1, 0.2, 0.3)
    gp = ctypes.cast(g, ctypes.c_void_p)
    calls = [
        L.lz_csr_spmm_axpby4(None, 4, 0, None, None, None, lz.LZ_F64, 16, 1.0, None, 1.0, 0.0, None, 0.0, None, None),
        L.lz_cheb_series_apply(None, 4, 0, None, None, None, lz.LZ_F64, 16, 2, LO, HI, gp, None, None, None),
        L.lz_block_lanczos_reorth_series(None, 4, 0, None, None, None, lz.LZ_F64, 16, 2, 0, None, None, None, None,
                                         None, 64, None, 2, 2, LO, HI, gp, None),
        L.lz_block_lanczos_reorth_resume_series(None, 4, 0, None, None, None, lz.LZ_F64, 16, 1, 2, 0, None, None, None,
                                                None, None, 64, None, 2, 2, LO, HI, gp, None),
    ]
    for rc in calls:
        assert rc != 0
        assert b"handle" in L.lz_last_error()
