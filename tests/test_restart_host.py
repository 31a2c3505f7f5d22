"""Host side of the thick restart (no GPU): lzh_ritz_pairs_dense,
lzh_restart_coeffs, lzh_restart_fill, and a small dense block Lanczos in NumPy
that restarts through them only and must end with P^T A P = T."""
import ctypes

import numpy as np
import pytest


def lanczos_cycle(D, Q, W, j0, m, b, alpha, beta, S=None):
    """Steps j0 .. m-1 of block Lanczos with two rounds of full reorthogonalisation on the
    dense D (fp64, sqrtm by eigh); step j0 subtracts [Q_0 .. Q_{j0-1}] S when S is given
    (the restarted step), Q_{j-1} beta_j otherwise.  Fills Q, alpha, beta[j0 .. m]; returns W."""
    def sqrtm_pair(G):
        w, U = np.linalg.eigh(0.5 * (G + G.T))
        return (U * np.sqrt(w)) @ U.T, (U / np.sqrt(w)) @ U.T

    for j in range(j0, m):
        beta[j], bi = sqrtm_pair(W.T @ W)
        Q[j] = W @ bi
        W = D @ Q[j]
        if S is not None and j == j0:
            W = W - np.concatenate(Q[:j0], axis=1) @ S
        elif j:
            W = W - Q[j - 1] @ beta[j]
        a = W.T @ Q[j]
        alpha[j] = 0.5 * (a + a.T)
        W = W - Q[j] @ alpha[j]
        P = np.concatenate(Q[:j + 1], axis=1)
        for _ in range(2):
            W = W - P @ (P.T @ W)
    beta[m] = sqrtm_pair(W.T @ W)[0]
    return W


def random_solve(n, b, m, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(-1, 1, (n, n))
    D = 0.5 * (D + D.T)
    Q, alpha, beta = [None] * m, np.zeros((m, b, b)), np.zeros((m + 1, b, b))
    W = lanczos_cycle(D, Q, rng.uniform(1, 2, (n, b)), 0, m, b, alpha, beta)
    return D, Q, alpha, beta, W


@pytest.mark.parametrize("m,b", [(4, 3), (6, 4), (3, 16)])
@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_ritz_pairs_dense_equals_ritz_pairs(lz, m, b, which):
    _, _, alpha, beta, _ = random_solve(120, b, m, 10 * m + b)
    nev = m * b - 1
    t0, S0, r0 = lz.ritz_pairs(m, b, alpha, beta, nev, which)
    t1, S1, r1 = lz.ritz_pairs_dense(m, b, lz.Assemble_T(m, b, alpha, beta), beta[m], nev, which)
    assert np.abs(t0 - t1).max() <= 1e-13 and np.abs(r0 - r1).max() <= 1e-13
    sign = np.sign(np.sum(S0 * S1, axis=0))
    assert np.abs(S0 - S1 * sign).max() <= 1e-13
    # and both are the eigenpairs of T
    T = lz.Assemble_T(m, b, alpha, beta)
    ev = np.linalg.eigvalsh(T)
    assert np.abs(t1 - (ev[:nev] if which == "smallest" else ev[::-1][:nev])).max() <= 1e-12
    assert np.abs(T @ S1 - S1 * t1).max() <= 1e-12
    assert np.abs(r1 - np.linalg.norm(beta[m] @ S1[-b:], axis=0)).max() <= 1e-13


@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_restart_coeffs(lz, which):
    m, b, r = 6, 4, 2
    _, _, alpha, beta, _ = random_solve(150, b, m, 77)
    T = lz.Assemble_T(m, b, alpha, beta)
    theta_k, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], which)
    ev, E = np.linalg.eigh(T)
    idx = np.arange(m * b) if which == "smallest" else np.arange(m * b)[::-1]
    Zk_ref = E[:, idx[:r * b]]
    assert np.abs(theta_k - ev[idx[:r * b]]).max() <= 1e-13
    # the compress layout: Z[c][j] = rows j b .., columns c b .. of Z_k
    Zk = Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)
    sign = np.sign(np.sum(Zk * Zk_ref, axis=0))
    assert np.abs(Zk * sign - Zk_ref).max() <= 1e-12
    assert np.abs(Zk.T @ Zk - np.eye(r * b)).max() <= 1e-13
    Sigma = beta[m] @ Zk[-b:]  # b x r b, with this call's signs
    for i in range(r):
        assert np.abs(sigma[i] - Sigma[:, i * b:(i + 1) * b].T).max() <= 1e-14
    # T_next: the diagonal, the mirrored arrow block, nothing else
    ref = np.zeros_like(T)
    ref[np.arange(r * b), np.arange(r * b)] = theta_k
    ref[r * b:(r + 1) * b, :r * b] = Sigma
    ref[:r * b, r * b:(r + 1) * b] = Sigma.T
    assert np.abs(Tn - ref).max() <= 1e-14
    assert (Tn[ref == 0] == 0).all()


def test_restart_fill_places_the_tail(lz):
    m, b, r = 5, 3, 2
    rng = np.random.default_rng(5)
    alpha, beta = rng.uniform(-1, 1, (m, b, b)), rng.uniform(-1, 1, (m + 1, b, b))
    Tn = np.zeros((m * b, m * b))
    lz.restart_fill(r, m, b, alpha, beta, Tn)
    ref = lz.Assemble_T(m, b, alpha, beta)
    ref[:r * b, :] = 0  # rows and columns of the kept part, the beta_r coupling included
    ref[:, :r * b] = 0
    assert np.array_equal(Tn, ref)


def test_dense_restart_end_to_end(lz):
    """n = 200, b = 4, m = 6, r = 2: a cycle, a restart through the host functions only, a
    continued cycle: P^T A P = T to 1e-11 and the basis is orthonormal."""
    n, b, m, r = 200, 4, 6, 2
    D, Q, alpha, beta, W = random_solve(n, b, m, 2026)
    T = lz.Assemble_T(m, b, alpha, beta)
    P = np.concatenate(Q, axis=1)
    assert np.abs(P.T @ D @ P - T).max() <= 1e-11
    for which in ("largest", "smallest"):  # two restarts in a row, one at each end
        theta_k, Z, sigma, Tn = lz.restart_coeffs(m, b, r, T, beta[m], which)
        Y = np.einsum("jri,cjid->crd", np.stack(Q), Z)  # what lz_panel_compress computes
        for c in range(r):
            Q[c] = Y[c]
        W = lanczos_cycle(D, Q, W, r, m, b, alpha, beta, S=sigma.reshape(r * b, b))
        T = lz.restart_fill(r, m, b, alpha, beta, Tn)
        P = np.concatenate(Q, axis=1)
        err = np.abs(P.T @ D @ P - T).max()
        print(f"{which}: max|P^T A P - T| = {err:.3e}, max|P^T P - I| = {np.abs(P.T @ P - np.eye(m * b)).max():.3e}")
        assert err <= 1e-11
        assert np.abs(P.T @ P - np.eye(m * b)).max() <= 1e-12
        # the residual estimate of the restarted T is the true residual norm
        theta, S, resid = lz.ritz_pairs_dense(m, b, T, beta[m], 3, which)
        X = P @ S
        assert np.abs(np.linalg.norm(D @ X - X * theta, axis=0) - resid).max() <= 1e-10


def test_argument_errors(lz):
    H = lz.host_lib()
    m, b, r = 3, 2, 1
    k = m * b
    T, bm = np.eye(k), np.eye(b)
    th, S, rs = np.empty(k), np.empty((k, k)), np.empty(k)
    Z, sg, Tn = np.empty((r, m, b, b)), np.empty((r, b, b)), np.empty((k, k))
    al, be = np.zeros((m, b, b)), np.zeros((m + 1, b, b))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert H.lzh_ritz_pairs_dense(m, b, p(T), p(bm), 2, 1, p(th), p(S), p(rs)) == 0
    assert H.lzh_ritz_pairs_dense(m, b, p(T), p(bm), k + 1, 1, p(th), p(S), p(rs)) == -1  # nev > m*b
    assert H.lzh_ritz_pairs_dense(m, b, p(T), p(bm), 0, 1, p(th), p(S), p(rs)) == -1
    assert H.lzh_ritz_pairs_dense(m, b, p(T), p(bm), 2, 2, p(th), p(S), p(rs)) == -1      # which
    assert H.lzh_ritz_pairs_dense(m, b, None, p(bm), 2, 1, p(th), p(S), p(rs)) == -1
    assert H.lzh_ritz_pairs_dense(m, b, p(T), None, 2, 1, p(th), p(S), p(rs)) == -1       # resid needs beta_m
    assert H.lzh_restart_coeffs(m, b, r, p(T), p(bm), 1, p(th), p(Z), p(sg), p(Tn)) == 0
    assert H.lzh_restart_coeffs(m, b, 0, p(T), p(bm), 1, p(th), p(Z), p(sg), p(Tn)) == -1  # r = 0
    assert H.lzh_restart_coeffs(m, b, m, p(T), p(bm), 1, p(th), p(Z), p(sg), p(Tn)) == -1  # r >= m
    assert H.lzh_restart_coeffs(m, b, r, p(T), p(bm), 3, p(th), p(Z), p(sg), p(Tn)) == -1
    assert H.lzh_restart_coeffs(m, b, r, p(T), None, 1, p(th), p(Z), p(sg), p(Tn)) == -1
    assert H.lzh_restart_fill(r, m, b, p(al), p(be), p(Tn)) == 0
    assert H.lzh_restart_fill(m, m, b, p(al), p(be), p(Tn)) == -1
    assert H.lzh_restart_fill(0, m, b, p(al), p(be), p(Tn)) == -1
    assert H.lzh_restart_fill(r, m, b, None, p(be), p(Tn)) == -1
    with pytest.raises(ValueError):
        lz.ritz_pairs_dense(m, b, T, bm, 2, "middle")
    with pytest.raises(lz.LanczosError):
        lz.restart_coeffs(m, b, m, T, bm)
