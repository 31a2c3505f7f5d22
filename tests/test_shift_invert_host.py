"""The host side of shift-and-invert eigsh, without a GPU: the largest-magnitude Ritz selection
(lzh_ritz_pairs_dense_mag, lzh_restart_coeffs_mag) against numpy.linalg.eigh, the order and its
tie rule, the argument errors, that the two older functions still reject which = 2 and 3, and
that every new symbol is declared, exported and bound.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2), (6, 4)]
NEW_HOST = ["lzh_ritz_pairs_dense_mag", "lzh_restart_coeffs_mag"]
NEW_HIP = ["lz_csr_spmm_resid", "lz_inverse_apply", "lz_block_lanczos_reorth_inverse",
           "lz_block_lanczos_reorth_resume_inverse"]


def random_T(m, b, seed):
    rng = np.random.default_rng(seed)
    k = m * b
    T = rng.uniform(-1, 1, (k, k))
    return 0.5 * (T + T.T), rng.uniform(-1, 1, (b, b))


def mag_order(ev):
    """|theta| descending, ties by theta ascending."""
    return sorted(range(len(ev)), key=lambda i: (-abs(ev[i]), ev[i]))


@pytest.mark.parametrize("m,b", SHAPES)
def test_ritz_pairs_mag_against_eigh(lz, m, b):
    T, bm = random_T(m, b, 10 * m + b)
    k = m * b
    ev, Z = np.linalg.eigh(T)
    order = mag_order(ev)
    for nev in (1, b + 1, k):
        theta, S, resid = lz.ritz_pairs_dense(m, b, T, bm, nev, "magnitude")
        assert np.abs(theta - ev[order[:nev]]).max() <= 1e-13
        assert (np.diff(np.abs(theta)) <= 0).all()
        for i in range(nev):  # an eigenvector up to its sign (random T: simple eigenvalues)
            z = Z[:, order[i]]
            assert min(np.abs(S[:, i] - z).max(), np.abs(S[:, i] + z).max()) <= 1e-10
            assert abs(resid[i] - np.linalg.norm(bm @ S[-b:, i])) <= 1e-14
            assert np.linalg.norm(T @ S[:, i] - theta[i] * S[:, i]) <= 1e-13
    # the same pairs as the two one-sided selections hold between them
    lo = lz.ritz_pairs_dense(m, b, T, bm, k, "smallest")[0]
    assert np.array_equal(np.sort(lz.ritz_pairs_dense(m, b, T, bm, k, "magnitude")[0]), lo)


def test_tie_rule(lz):
    """A diagonal T has its entries as exact eigenvalues: -t comes before +t."""
    T = np.diag([2.0, -2.0, 1.0, -1.0, 0.5, -3.0])
    theta, S, _ = lz.ritz_pairs_dense(3, 2, T, np.eye(2), 6, "magnitude")
    assert theta.tolist() == [-3.0, -2.0, 2.0, -1.0, 1.0, 0.5]
    assert np.array_equal(np.abs(S), np.eye(6)[:, [5, 1, 0, 3, 2, 4]])
    theta_k, Z, _, _ = lz.restart_coeffs(3, 2, 2, T, np.eye(2), "magnitude")
    assert theta_k.tolist() == [-3.0, -2.0, 2.0, -1.0]


@pytest.mark.parametrize("m,b", SHAPES)
def test_restart_coeffs_mag(lz, m, b):
    T, bm = random_T(m, b, 7 * m + b)
    k = m * b
    for r in (1, m - 1):
        rb = r * b
        theta, S, _ = lz.ritz_pairs_dense(m, b, T, bm, rb, "magnitude")
        theta_k, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, bm, "magnitude")
        assert np.array_equal(theta_k, theta)
        Zk = Z.transpose(1, 2, 0, 3).reshape(k, rb)  # Z[c][j] = rows j, columns c of Z_k
        assert np.array_equal(Zk, S)
        Sigma = bm @ Zk[-b:, :]
        for i in range(r):
            assert np.abs(sigma[i] - Sigma[:, i * b:(i + 1) * b].T).max() <= 1e-15
        want = np.zeros((k, k))
        want[np.arange(rb), np.arange(rb)] = theta_k
        want[rb:rb + b, :rb] = Sigma  # the arrow: block row r, mirrored into block column r
        want[:rb, rb:rb + b] = Sigma.T
        assert np.abs(Tn - want).max() <= 1e-15 and np.array_equal(Tn, Tn.T)
        # thick restart's relation on the projected matrix: Z_k^T T Z_k = diag(theta_k)
        assert np.abs(Zk.T @ T @ Zk - np.diag(theta_k)).max() <= 1e-13


def test_argument_errors(lz):
    L = lz.host_lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    m, b = 3, 2
    k = m * b
    T, bm = random_T(m, b, 1)
    th, S, res = np.empty(k), np.empty((k, k)), np.empty(k)
    Z, sg, Tn = np.empty((m, m, b, b)), np.empty((m, b, b)), np.empty((k, k))
    ok = L.lzh_ritz_pairs_dense_mag(m, b, p(T), p(bm), k, p(th), p(S), p(res))
    assert ok == 0
    assert L.lzh_ritz_pairs_dense_mag(m, b, p(T), None, k, p(th), p(S), None) == 0  # resid and beta_m may be NULL
    for args in [(0, b, p(T), p(bm), 1, p(th), p(S), p(res)), (m, 0, p(T), p(bm), 1, p(th), p(S), p(res)),
                 (m, b, None, p(bm), 1, p(th), p(S), p(res)), (m, b, p(T), p(bm), 0, p(th), p(S), p(res)),
                 (m, b, p(T), p(bm), k + 1, p(th), p(S), p(res)), (m, b, p(T), p(bm), 1, None, p(S), p(res)),
                 (m, b, p(T), p(bm), 1, p(th), None, p(res)), (m, b, p(T), None, 1, p(th), p(S), p(res))]:
        assert L.lzh_ritz_pairs_dense_mag(*args) == -1
    assert L.lzh_restart_coeffs_mag(m, b, 1, p(T), p(bm), p(th), p(Z), p(sg), p(Tn)) == 0
    for args in [(m, b, 0, p(T), p(bm), p(th), p(Z), p(sg), p(Tn)), (m, b, m, p(T), p(bm), p(th), p(Z), p(sg), p(Tn)),
                 (m, b, 1, None, p(bm), p(th), p(Z), p(sg), p(Tn)), (m, b, 1, p(T), None, p(th), p(Z), p(sg), p(Tn)),
                 (m, b, 1, p(T), p(bm), None, p(Z), p(sg), p(Tn)), (m, b, 1, p(T), p(bm), p(th), None, p(sg), p(Tn)),
                 (m, b, 1, p(T), p(bm), p(th), p(Z), None, p(Tn)), (m, b, 1, p(T), p(bm), p(th), p(Z), p(sg), None)]:
        assert L.lzh_restart_coeffs_mag(*args) == -1
    # the older functions: which is still 0 or 1
    for which in (2, 3, -1):
        assert L.lzh_ritz_pairs_dense(m, b, p(T), p(bm), k, which, p(th), p(S), p(res)) == -1
        assert L.lzh_restart_coeffs(m, b, 1, p(T), p(bm), which, p(th), p(Z), p(sg), p(Tn)) == -1
    # the wrappers
    for which in ("middle", "both", 2):
        with pytest.raises(ValueError):
            lz.ritz_pairs_dense(m, b, T, bm, 2, which)
        with pytest.raises(ValueError):
            lz.restart_coeffs(m, b, 1, T, bm, which)
    with pytest.raises(ValueError):
        lz.ritz_pairs(m, b, np.zeros((m, b, b)), np.zeros((m + 1, b, b)), 2, "magnitude")  # (tridiagonal form: no)
    with pytest.raises(ValueError):
        lz.ritz_pairs_dense(m, b, T[:-1], bm, 2, "magnitude")
    with pytest.raises(lz.LanczosError):
        lz.restart_coeffs(m, b, m, T, bm, "magnitude")
    with pytest.raises(lz.LanczosError):
        lz.ritz_pairs_dense(m, b, T, bm, k + 1, "magnitude")


def test_abi(lz):
    """Every new symbol: declared in its header, exported by its library, bound in its table."""
    for header, lib, table, names in [("lz_host.h", lz.host_lib(), lz.HOST_SYMBOLS, NEW_HOST),
                                      ("lz_hip.h", lz.hip_lib(), lz.HIP_SYMBOLS, NEW_HIP)]:
        text = open(os.path.join(ROOT, "include", header)).read()
        bound = {name: args for name, _, args in table}
        for name in names:
            decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
            assert decl, f"{name} is not declared in include/{header}"
            assert hasattr(lib, name), f"{name} is not exported"
            assert name in bound and len(bound[name]) == decl.group(1).count(",") + 1, f"{name}: arguments bound"
    text = open(os.path.join(ROOT, "include", "lz_hip.h")).read()
    assert "} lz_inverse;" in text and "} lz_inverse_info;" in text
    assert re.search(r"LZ_K_RESID = 0x4000\b", text) and lz.LZ_K_RESID == 0x4000
    # the structs as the header lays them out
    assert ctypes.sizeof(lz.Inverse) == 40 and lz.Inverse.opts.offset == 16
    assert ctypes.sizeof(lz.InverseInfo) == 48 and lz.InverseInfo.worst.offset == 40


def test_signatures(lz):
    sig = inspect.signature(lz.Handle.eigsh).parameters
    assert sig["sigma"].default is None and sig["inner"].default == "minres"
    assert sig["inner_tol"].default is None and sig["inner_max_iter"].default is None
    assert list(sig)[:14] == ["self", "A", "nev", "which", "b", "m", "keep", "tol", "max_cycles", "B", "lc", "passes",
                              "filter_degree", "cut"], "the existing arguments keep their places"
    for name in ("block_lanczos_reorth", "block_lanczos_reorth_resume", "_reorth_op"):
        assert inspect.signature(getattr(lz.Handle, name)).parameters["inverse"].default is None
    assert callable(lz.Handle.inverse_apply) and callable(lz.Handle.spmm_resid)
    assert 0.0 < lz.INNER_TOL_FACTOR <= 1.0
