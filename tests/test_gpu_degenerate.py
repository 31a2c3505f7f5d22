"""Never silently wrong, on the device: Handle.eigsh (plain, filtered, sigma=), eigsh_interval and
svds on repeated eigenvalues, clusters, rank-deficient start blocks, low-rank operators and
exhausted Krylov spaces, in both precisions.  The contract, the verification on the dense fp64
operator and where gap / orth come from are those of test_degenerate_driver.py (its docstring),
whose helpers run here unchanged; every operator has n <= 1024 and the host reference is NumPy's
dense fp64 eigvalsh / svd.  No input here can fault a kernel: NaN / Inf arithmetic is the worst
that a singular Gram leads to.
"""
import numpy as np
import pytest

from test_degenerate_driver import (cheb_dense, copies, deficient_blocks, ends, from_dense, low_rank,
                                    never_silently_wrong, restate, restate_svds, two_blocks, verify_eig, verify_svd)
from test_gpu_restart import dense, host_panel

pytestmark = pytest.mark.gpu

LC = 5
F64, F32 = np.float64, np.float32

# name: (n0, copies, planted rows, shift, dtype, b, m, keep, nev, which, tol)
HEALTHY = {
    "H1": (256, 4, 4, 0.0, F64, 16, 6, 2, 16, "largest", 1e-10),
    "H2": (512, 2, 8, 0.0, F64, 16, 6, 2, 16, "largest", 1e-10),
    "H3": (160, 5, 2, 0.0, F64, 5, 12, 5, 10, "largest", 1e-10),   # multiplicity = b
    "H4": (64, 16, 1, 0.0, F64, 16, 6, 2, 16, "largest", 1e-10),   # multiplicity = b = nev
    "H5": (256, 4, 4, 1e-9, F64, 16, 6, 2, 16, "largest", 1e-10),  # four eigenvalues within 3e-9
    "H6": (256, 4, 4, 0.0, F32, 32, 4, 1, 16, "largest", 2e-5),
    "H7": (256, 4, 4, 0.0, F64, 16, 8, 3, 16, "smallest", 1e-8),
}


class Problem:
    pass


_cache = {}


def healthy(lz, name):
    """The operator, its dense copy and spectrum, uniform_B and the restatement's (cycles, gap,
    orth), once per case."""
    if name not in _cache:
        n0, k, npl, shift, npdt, b, m, r, nev, which, tol = HEALTHY[name]
        s = Problem()
        s.A, s.D = copies(lz, n0, k, npl, npdt, shift)
        s.n, s.npdt = s.A.n, npdt
        s.ev = np.linalg.eigvalsh(s.D)
        s.Bh = lz.uniform_B(s.n, b, dtype=npdt)
        s.cycles, s.gap, s.orth = restate(s.D, s.Bh, b, m, r, nev, which, npdt, tol)
        s.Ad = lz.CsrDevice.from_host(s.A)
        _cache[name] = s
    return _cache[name]


def lap20(lz):
    if "lap" not in _cache:
        s = Problem()
        s.A = lz.gen_laplace2d(20, 20)
        s.D, s.n, s.npdt = dense(s.A), s.A.n, F64
        s.ev = np.linalg.eigvalsh(s.D)
        s.Bh = lz.uniform_B(s.n, 16)
        s.Ad = lz.CsrDevice.from_host(s.A)
        _cache["lap"] = s
    return _cache["lap"]


def arithmetic(lz, npdt):
    """(gap, orth) for an input that has no healthy restatement of its own: H1's (fp64) or H6's
    (fp32), the same size and precision."""
    s = healthy(lz, "H1" if npdt is F64 else "H6")
    return s.gap, s.orth


def panel(out, n, b, nev, key="V", stride="vstride"):
    """The nev returned vectors as fp64 columns (cols, where the solve returns it, picks them)."""
    nch = max(1, -(-nev // b))
    vs = out[stride]
    X = host_panel(out[key][:nch * vs], nch, vs, n, b)
    return X[:, out["cols"]] if "cols" in out else X[:, :nev]


def dev(torch, B):
    return torch.from_numpy(np.ascontiguousarray(B)).cuda()


def eig_check(name, s, b, nev, tol, gap, orth, which="largest", sigma=None, window=None):
    def check(out):
        want = ends(s.ev, nev, which, sigma) if window is None else s.ev[(s.ev >= window[0]) & (s.ev <= window[1])]
        verify_eig(name, s.D, panel(out, s.n, b, len(out["theta"])), out["theta"], want, tol, out["scale"], gap, orth)
    return check


def svd_check(name, S, b, k, tol, gap, orth):
    def check(out):
        verify_svd(name, S, panel(out, S.shape[0], b, k, "U", "ustride"), panel(out, S.shape[1], b, k), out["s"], tol,
                   gap, orth)
    return check


# -------------------------------------------------------- healthy but hard
@pytest.mark.parametrize("name", list(HEALTHY))
def test_repeated_eigenvalues_converge(lz, handle, torch_cuda, name):
    """Every eigenvalue with multiplicity k (H5: a cluster of width 3e-9): all nev copies, in at
    most twice the restatement's cycles."""
    n0, k, npl, shift, npdt, b, m, r, nev, which, tol = HEALTHY[name]
    s = healthy(lz, name)
    out = handle.eigsh(s.Ad, nev, which=which, b=b, m=m, keep=r, tol=tol, max_cycles=2 * s.cycles,
                       B=dev(torch_cuda, s.Bh), lc=LC, passes=2)
    print(f"{name}: device {out['cycles']} cycles (restatement {s.cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * s.cycles
    assert set(out) == {"theta", "resid", "V", "vstride", "cycles", "n_spmm", "converged", "history", "scale"}
    eig_check(name, s, b, nev, tol, s.gap, s.orth, which)(out)


def test_paired_eigenvalues_sigma(lz, handle, torch_cuda):
    """The 20 x 20 Laplacian, whose eigenvalues come in pairs: the six nearest sigma = 0."""
    s = lap20(lz)
    b, m, r, nev, tol = 16, 6, 2, 6, 1e-10
    Mi = np.linalg.inv(s.D)
    scale = max(abs(x) for x in lz.gershgorin(s.Ad))
    cycles, gap, orth = restate(s.D, s.Bh, b, m, r, nev, "largest", F64, tol, mul=lambda Q: Mi @ Q,
                                rr=(lambda lam: np.argsort(np.abs(lam), kind="stable"), scale))
    out = handle.eigsh(s.Ad, nev, b=b, m=m, keep=r, tol=tol, sigma=0.0, inner="block", max_cycles=2 * cycles,
                       B=dev(torch_cuda, s.Bh), lc=LC)
    print(f"sigma = 0: device {out['cycles']} cycles (restatement {cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    eig_check("sigma = 0", s, b, nev, tol, gap, orth, sigma=0.0)(out)


def test_paired_eigenvalues_filtered(lz, handle, torch_cuda):
    s = lap20(lz)
    b, m, r, nev, tol = 16, 6, 2, 6, 1e-10
    out = handle.eigsh(s.Ad, nev, which="smallest", b=b, m=m, keep=r, tol=tol, filter_degree=12, max_cycles=40,
                       B=dev(torch_cuda, s.Bh), lc=LC)
    assert out["converged"] is True
    if out["filter"] is None:  # the unfiltered solve already met tol: the plain solve's figures
        cycles, (_, gap, orth) = 0, restate(s.D, s.Bh, b, m, r, nev, "smallest", F64, tol)
    else:
        P = cheb_dense(s.D, out["filter"])
        cycles, gap, orth = restate(s.D, s.Bh, b, m, r, nev, "largest", F64, tol, mul=lambda Q: P @ Q,
                                    rr=(lambda lam: np.argsort(lam, kind="stable"), out["scale"]))
    print(f"filtered: device {out['cycles']} cycles (restatement {cycles})")
    assert out["cycles"] <= 2 * cycles
    eig_check("filtered", s, b, nev, tol, gap, orth, "smallest")(out)


@pytest.mark.parametrize("shape", ["tall", "wide"])
def test_svds_repeated_singular_values(lz, handle, torch_cuda, shape):
    """H1's matrix over a zero block (tall) and that transposed (wide): every singular value four times."""
    s = healthy(lz, "H1")
    b, m, r, k, tol = 16, 6, 2, 16, 1e-10
    S = np.vstack([s.D, np.zeros((200, s.n))])
    S = S if shape == "tall" else np.ascontiguousarray(S.T)
    cycles, gap, orth = restate_svds(S, s.Bh, b, m, r, k, F64, tol)
    Ad = lz.CsrDevice.from_host(from_dense(lz, S), n_cols=S.shape[1])
    out = handle.svds(Ad, k, b=b, m=m, keep=r, tol=tol, max_cycles=2 * cycles, B=dev(torch_cuda, s.Bh), lc=LC)
    print(f"svds {shape}: device {out['cycles']} cycles (restatement {cycles})")
    assert out["converged"] is True and out["cycles"] <= 2 * cycles
    svd_check(f"svds {shape}", S, b, k, tol, gap, orth)(out)


# ---------------------------------------------------------------- deficient
START = [("D1", "H1", True), ("D1", "H6", True), ("D2", "H1", True), ("D2", "H6", False), ("D3", "H1", True),
         ("D3", "H6", False), ("D4", "H1", False)]


@pytest.mark.parametrize("case,on,must_raise", START, ids=[f"{c}-{'f64' if o == 'H1' else 'f32'}" for c, o, _ in START])
def test_deficient_start_block(lz, handle, torch_cuda, case, on, must_raise):
    """A zero column, a duplicated column, rank 1, a column duplicated to 1e-7, on H1 (fp64) and
    H6 (fp32): refused where the table of DESIGN.md 28 shows a gap, contract items 1 - 3 elsewhere."""
    n0, k, npl, shift, npdt, b, m, r, nev, which, tol = HEALTHY[on]
    s = healthy(lz, on)
    B = dev(torch_cuda, deficient_blocks(s.Bh)[case])
    never_silently_wrong(lz, f"{case} {on}", lambda: handle.eigsh(s.Ad, nev, which=which, b=b, m=m, keep=r, tol=tol,
                                                                  max_cycles=2 * s.cycles, B=B, lc=LC),
                         eig_check(case, s, b, nev, tol, s.gap, s.orth, which), must_raise=must_raise)


@pytest.mark.parametrize("case,on,must_raise", [("D1", "H1", True), ("D2", "H1", True), ("D1", "H6", True),
                                                ("D2", "H6", False)])
def test_svds_deficient_start_block(lz, handle, torch_cuda, case, on, must_raise):
    n0, k, npl, shift, npdt, b, m, r, nev, which, tol = HEALTHY[on]
    s = healthy(lz, on)
    B = dev(torch_cuda, deficient_blocks(s.Bh)[case])
    gap, orth = arithmetic(lz, npdt)
    never_silently_wrong(lz, f"svds {case} {on}", lambda: handle.svds(s.Ad, nev, b=b, m=m, keep=r, tol=tol,
                                                                      max_cycles=12, B=B, lc=LC),
                         svd_check(case, s.D, b, nev, tol, gap, orth), must_raise=must_raise,
                         finite=("s", "resid", "est", "history"))


FORMS = {  # the forms that measure their residuals on A; the Rayleigh-Ritz step still assumes an orthonormal panel
    "filtered": lambda h, Ad, B, kw: h.eigsh(Ad, 6, which="smallest", filter_degree=12, B=B, **kw),
    "interval": lambda h, Ad, B, kw: h.eigsh_interval(Ad, 0.3, 0.9, block=kw.pop("b"), B=B, **kw),
    "sigma": lambda h, Ad, B, kw: h.eigsh(Ad, 6, sigma=0.0, inner="block", B=B, **kw),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_d2_other_forms(lz, handle, torch_cuda, form):
    """The duplicated column on the 20 x 20 Laplacian through filtered eigsh, eigsh_interval and sigma=."""
    s = lap20(lz)
    B = dev(torch_cuda, deficient_blocks(s.Bh)["D2"])
    kw = dict(b=16, m=6, keep=2, tol=1e-10, max_cycles=8, lc=LC)
    gap, orth = arithmetic(lz, F64)
    which, sigma, window = {"filtered": ("smallest", None, None), "interval": ("largest", None, (0.3, 0.9)),
                            "sigma": ("largest", 0.0, None)}[form]
    never_silently_wrong(lz, f"D2 {form}", lambda: FORMS[form](handle, s.Ad, B, kw),
                         eig_check(f"D2 {form}", s, 16, 6, 1e-10, gap, orth, which, sigma, window), must_raise=True)


@pytest.mark.parametrize("npdt", [F64, F32], ids=["f64", "f32"])
def test_d5_low_rank_operator(lz, handle, torch_cuda, npdt):
    """blockdiag(S40, 0) at n = 1024: 984 empty rows, rank 40 < m b - b; the Krylov space of any
    start block is exhausted inside the first cycle."""
    s = Problem()
    s.A, s.D = low_rank(lz, 1024, 40, npdt)
    s.n, s.ev = 1024, np.linalg.eigvalsh(s.D)
    Ad = lz.CsrDevice.from_host(s.A)
    b, m, r, nev, tol = (16, 6, 2, 16, 1e-10) if npdt is F64 else (32, 4, 1, 16, 2e-5)
    gap, orth = arithmetic(lz, npdt)
    never_silently_wrong(lz, "D5", lambda: handle.eigsh(Ad, nev, b=b, m=m, keep=r, tol=tol, max_cycles=8, lc=LC),
                         eig_check("D5", s, b, nev, tol, gap, orth))
    never_silently_wrong(lz, "D5 svds", lambda: handle.svds(Ad, nev, b=b, m=m, keep=r, tol=tol, max_cycles=8, lc=LC),
                         svd_check("D5 svds", s.D, b, nev, tol, gap, orth),
                         finite=("s", "resid", "est", "history"))


@pytest.mark.parametrize("form", list(FORMS))
def test_d5_other_forms(lz, handle, torch_cuda, form):
    """The low-rank operator (n = 400 for sigma=: (A + 0.5 I)^-1 has a 360-fold eigenvalue) through
    the other forms, from the default start block."""
    s = Problem()
    s.n = 400 if form == "sigma" else 1024
    s.A, s.D = low_rank(lz, s.n, 40)
    s.ev = np.linalg.eigvalsh(s.D)
    Ad = lz.CsrDevice.from_host(s.A)
    kw = dict(b=16, m=6, keep=2, tol=1e-10, max_cycles=6, lc=LC)
    gap, orth = arithmetic(lz, F64)
    solve = {"filtered": lambda: handle.eigsh(Ad, 6, which="smallest", filter_degree=12, **kw),
             "interval": lambda: handle.eigsh_interval(Ad, 1.0, 2.0, block=16, m=6, keep=2, max_cycles=6, lc=LC),
             "sigma": lambda: handle.eigsh(Ad, 6, sigma=-0.5, **kw)}[form]
    which, sigma, window = {"filtered": ("smallest", None, None), "interval": ("largest", None, (1.0, 2.0)),
                            "sigma": ("largest", -0.5, None)}[form]
    never_silently_wrong(lz, f"D5 {form}", solve, eig_check(f"D5 {form}", s, 16, 6, 1e-10, gap, orth, which, sigma, window))


def test_d6_start_block_inside_an_invariant_subspace(lz, handle, torch_cuda):
    """blockdiag(A1 of 48 rows, A2) with B zero outside A1's rows: raising or re-randomising
    correctly both pass; returning A1's pairs as A's outermost does not."""
    s = Problem()
    s.A, s.D = two_blocks(lz, 1024, 48)
    s.n, s.ev = 1024, np.linalg.eigvalsh(s.D)
    B = lz.uniform_B(s.n, 16)
    B[48:] = 0
    gap, orth = arithmetic(lz, F64)
    never_silently_wrong(lz, "D6", lambda: handle.eigsh(lz.CsrDevice.from_host(s.A), 16, b=16, m=6, keep=2, tol=1e-10,
                                                        max_cycles=8, B=dev(torch_cuda, B), lc=LC),
                         eig_check("D6", s, 16, 16, 1e-10, gap, orth))


def test_d8_svds_few_rows(lz, handle, torch_cuda):
    """svds of a 600 x 400 matrix with 24 non-empty rows, k = 8: rank 24 < m b - b."""
    rng = np.random.default_rng(8)
    S = np.zeros((600, 400))
    S[::25] = rng.uniform(-1, 1, (24, 400))
    Ad = lz.CsrDevice.from_host(from_dense(lz, S), n_cols=400)
    gap, orth = arithmetic(lz, F64)
    never_silently_wrong(lz, "D8", lambda: handle.svds(Ad, 8, b=16, m=6, keep=2, tol=1e-10, max_cycles=8, lc=LC),
                         svd_check("D8", S, 16, 8, 1e-10, gap, orth),
                         finite=("s", "resid", "est", "history"))


@pytest.mark.parametrize("npdt", [F64, F32], ids=["f64", "f32"])
def test_d7_panel_wider_than_the_operator(lz, handle, torch_cuda, npdt):
    """m * b = 96 > n = 40 is refused at argument time in every form; svds by min(R, C)."""
    A, _ = copies(lz, 40, 1, 0, npdt)
    Ad = lz.CsrDevice.from_host(A)
    S = np.zeros((100, 40))
    S[np.arange(100), np.arange(100) % 40] = 1.0 + np.arange(100)
    tall = lz.CsrDevice.from_host(from_dense(lz, S, npdt), n_cols=40)
    wide = lz.CsrDevice.from_host(from_dense(lz, np.ascontiguousarray(S.T), npdt), n_cols=100)
    kw = dict(b=16, m=6, keep=2)
    for solve in (lambda: handle.eigsh(Ad, 8, **kw), lambda: handle.eigsh(Ad, 8, filter_degree=8, **kw),
                  lambda: handle.eigsh(Ad, 8, sigma=0.5, **kw),
                  lambda: handle.eigsh_interval(Ad, 0.1, 0.4, block=16, m=6, keep=2),
                  lambda: handle.svds(tall, 8, **kw), lambda: handle.svds(wide, 8, **kw)):
        with pytest.raises(lz.LanczosError, match=r"m \* b = 96 > n = 40"):
            solve()
