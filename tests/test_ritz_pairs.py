"""lzh_ritz_pairs (host): Ritz values, the eigenvectors of T and the residual
estimate ||beta_m S_last||, on random block-tridiagonal T."""
import numpy as np
import pytest


def random_T(m, b, seed):
    rng = np.random.default_rng(seed)
    sym = lambda x: 0.5 * (x + x.transpose(0, 2, 1))
    alpha = sym(rng.uniform(-1, 1, (m, b, b)))
    beta = sym(rng.uniform(-1, 1, (m + 1, b, b)))
    return alpha, beta


@pytest.mark.parametrize("m,b", [(5, 3), (4, 16)])
@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_ritz_pairs(lz, m, b, which):
    alpha, beta = random_T(m, b, 7 * m + b)
    k = m * b
    T = lz.Assemble_T(m, b, alpha, beta)
    assert np.array_equal(T, T.T)
    tol = 1e-12 * np.linalg.norm(T, 2)
    ev = np.linalg.eigvalsh(T)
    for nev in (1, 4, k):
        theta, S, resid = lz.ritz_pairs(m, b, alpha, beta, nev, which)
        want = ev[:nev] if which == "smallest" else ev[::-1][:nev]
        assert np.abs(theta - want).max() <= tol
        assert np.abs(T @ S - S * theta).max() <= tol
        assert np.abs(S.T @ S - np.eye(nev)).max() <= 1e-12
        est = np.linalg.norm(beta[m] @ S[-b:, :], axis=0)
        assert np.abs(resid - est).max() <= 1e-12 * np.linalg.norm(beta[m], 2)


def test_ritz_pairs_residual_is_the_true_one(lz):
    """With an orthonormal Lanczos basis of a real operator the estimate is the true
    residual norm: run the block recurrence in NumPy and compare."""
    rng = np.random.default_rng(3)
    n, b, m = 60, 3, 6
    A = rng.uniform(-1, 1, (n, n))
    A = A + A.T
    Q, _ = np.linalg.qr(rng.uniform(-1, 1, (n, b)))
    P, alpha, beta = [Q], [], [np.eye(b)]
    W = None
    for j in range(m):
        W = A @ P[j] - (P[j - 1] @ beta[j] if j else 0)
        a = P[j].T @ W
        alpha.append(0.5 * (a + a.T))
        W = W - P[j] @ alpha[j]
        Pm = np.concatenate(P, axis=1)
        W = W - Pm @ (Pm.T @ W)
        W = W - Pm @ (Pm.T @ W)
        w, U = np.linalg.eigh(W.T @ W)
        beta.append((U * np.sqrt(w)) @ U.T)
        P.append(W @ ((U / np.sqrt(w)) @ U.T))
    Pm = np.concatenate(P[:m], axis=1)
    theta, S, resid = lz.ritz_pairs(m, b, np.array(alpha), np.array(beta), 5, "largest")
    X = Pm @ S
    true = np.linalg.norm(A @ X - X * theta, axis=0)
    assert np.abs(true - resid).max() <= 1e-10 * np.abs(A).sum(axis=0).max()


def test_ritz_pairs_argument_checks(lz):
    alpha, beta = random_T(3, 2, 1)
    with pytest.raises(lz.LanczosError):
        lz.ritz_pairs(3, 2, alpha, beta, 7, "largest")  # nev > m*b
    with pytest.raises(ValueError):
        lz.ritz_pairs(3, 2, alpha, beta[:3], 2, "largest")  # beta without the beta_m block
    with pytest.raises(ValueError):
        lz.ritz_pairs(3, 2, alpha, beta, 2, "middle")
