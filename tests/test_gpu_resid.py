"""The residual store: R = A X - X diag(theta) with the dots [R.R | R.X] in one pass
(lz_csr_spmm_resid, SegStore::ShiftDots of k_spmm_seg, LZ_K_RESID).

R: NumPy fp64 on the exact (dtype-rounded) inputs, theta rounded to the dtype once as the kernel
does; per element
  |gpu - ref| <= (nnz_row + 3) eps (sum_j |a_ij| |x_j| + |theta_c| |x_i|),
the forward bound of a sum of nnz_row + 1 terms and the two fused multiply-adds behind it.  Dots:
against the fp64 column sums of the device's own R, as test_gpu_kpm's run_axpby_dots bounds them.
With every theta equal the call is spmm_axpby_dots(1, X, -theta, 0) bit for bit; the fused and the
two-launch forms store the same R; X is read only; two runs give the same bits.
"""
import numpy as np
import pytest

from test_gpu_cheb import csr, fused_operator, tile_runs
from test_gpu_kpm import dots_ok, nan_dots
from test_gpu_restart import f64

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EPS = {F64: float(np.finfo(F64).eps), F32: float(np.finfo(F32).eps)}
NAMES = ["n1", "n47", "n48", "n49", "n4099", "long_row"]
FUSED = [(16, F64), (32, F32)]
TWO_LAUNCH = [(5, F64), (4, F32)]

_ops = {}


def operator(lz, name, dtype):
    """The operator, its device copy and |A|: made once per (name, dtype)."""
    key = (name, dtype)
    if key not in _ops:
        A = fused_operator(lz, name, dtype)
        _ops[key] = (A, lz.CsrDevice.from_host(A), csr(A), abs(csr(A)))
    return _ops[key]


def inputs(torch, A, b, dtype, equal=None):
    rng = np.random.default_rng(3000 + A.n + b)
    Xh = rng.uniform(-1, 1, (A.n, b)).astype(dtype)
    th = rng.uniform(-2, 2, b) if equal is None else np.full(b, float(equal))
    return Xh, th, torch.from_numpy(Xh).cuda(), torch.from_numpy(th).cuda()


def run_resid(lz, handle, torch, name, b, dtype, fused):
    A, Ad, S, Sa = operator(lz, name, dtype)
    Xh, th, X, theta = inputs(torch, A, b, dtype)
    R, dots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    handle.spmm_resid(Ad, X, theta, R, dots=dots)
    k = handle.last_kernel()[0]
    if fused:
        runs = tile_runs(A, 48)
        assert (runs > 768).sum() >= 1 if name == "long_row" else (runs <= 768).all()
        assert k == lz.LZ_K_SEG768 | lz.LZ_K_RESID, f"kernel id {k:#x}"
    else:
        assert k & (lz.LZ_K_RESID | lz.LZ_K_AX3 | lz.LZ_K_DOT) == 0, f"kernel id {k:#x}"
    thr = f64(th.astype(dtype))  # rounded to the dtype once
    ref = S @ f64(Xh) - f64(Xh) * thr
    nnz_row = np.diff(A.row_ptr)[:, None]
    bound = (nnz_row + 3) * EPS[dtype] * (Sa @ np.abs(f64(Xh)) + np.abs(thr) * np.abs(f64(Xh)))
    got = f64(R.cpu().numpy())
    assert np.isfinite(got).all(), "NaN / Inf in R"
    err = np.abs(got - ref)
    print(f"spmm_resid {name} b={b} {dtype.__name__}: kernel {k:#x}, max err {err.max():.3e}, "
          f"max err/bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= bound).all()
    dots_ok(dots, R, X, f"spmm_resid {name} b={b} {dtype.__name__}")
    assert torch.equal(X, torch.from_numpy(Xh).cuda()), "X is read only"
    assert torch.equal(theta, torch.from_numpy(th).cuda()), "theta is read only"
    # a second run: the same bits
    R2, dots2 = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    handle.spmm_resid(Ad, X, theta, R2, dots=dots2)
    assert torch.equal(R, R2) and torch.equal(dots, dots2)
    return R, dots


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("b,dtype", FUSED)
def test_resid_fused(lz, handle, torch_cuda, monkeypatch, b, dtype, name):
    """128-byte rows: the residual and its dots leave k_spmm_seg's store.  47 / 48 / 49: the
    48-row tile edge; long_row: the MODE 1 store.  LZ_AX3=0: the two-launch form, the same R."""
    R, dots = run_resid(lz, handle, torch_cuda, name, b, dtype, True)
    A, Ad, _, _ = operator(lz, name, dtype)
    _, _, X, theta = inputs(torch_cuda, A, b, dtype)
    with monkeypatch.context() as mp:
        mp.setenv("LZ_AX3", "0")
        R2, dots2 = torch_cuda.full_like(X, float("nan")), nan_dots(torch_cuda, 1, b)
        handle.spmm_resid(Ad, X, theta, R2, dots=dots2)
        k = handle.last_kernel()[0]
    assert k == lz.LZ_K_SEG768, f"kernel id {k:#x}"
    assert torch_cuda.equal(R, R2), "fused and two-launch: the same bits in R"
    dots_ok(dots2, R2, X, f"two-launch {name}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("b,dtype", TWO_LAUNCH)
def test_resid_two_launch(lz, handle, torch_cuda, b, dtype, name):
    """Rows that are not 128 bytes: spmm, the row-local pass, the streaming dots."""
    run_resid(lz, handle, torch_cuda, name, b, dtype, False)


@pytest.mark.parametrize("name", ["n49", "long_row"])
@pytest.mark.parametrize("b,dtype", FUSED + TWO_LAUNCH)
def test_equal_theta_is_axpby_dots(lz, handle, torch_cuda, b, dtype, name):
    torch = torch_cuda
    A, Ad, _, _ = operator(lz, name, dtype)
    t = 0.3172
    _, _, X, theta = inputs(torch, A, b, dtype, equal=t)
    R, dots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    Y, ydots = torch.full_like(X, float("nan")), nan_dots(torch, 1, b)
    handle.spmm_resid(Ad, X, theta, R, dots=dots)
    handle.spmm_axpby_dots(Ad, 1.0, X, -t, 0.0, None, Y, dots=ydots)
    assert torch.equal(R, Y) and torch.equal(dots, ydots)


def test_unaligned_blocks_take_the_two_launch_form(lz, handle, torch_cuda):
    """X and R 8 bytes off a 16-byte boundary at the fused shape: no fused store (the SpMM is then
    the element-wise kernel, which sums a row in another order), R within the same forward bound."""
    torch = torch_cuda
    A, Ad, S, Sa = operator(lz, "n4099", F64)
    Xh, th, X, theta = inputs(torch, A, 16, F64)
    Xo = torch.empty(A.n * 16 + 1, dtype=X.dtype, device="cuda")[1:].view(A.n, 16)
    Ro = torch.full((A.n * 16 + 1,), float("nan"), dtype=X.dtype, device="cuda")[1:].view(A.n, 16)
    Xo.copy_(X)
    assert Xo.data_ptr() % 16 == 8
    dots = nan_dots(torch, 1, 16)
    handle.spmm_resid(Ad, Xo, theta, Ro, dots=dots)
    assert handle.last_kernel()[0] & lz.LZ_K_RESID == 0
    bound = (np.diff(A.row_ptr)[:, None] + 3) * EPS[F64] * (Sa @ np.abs(Xh) + np.abs(th) * np.abs(Xh))
    assert (np.abs(f64(Ro.cpu().numpy()) - (S @ Xh - Xh * th)) <= bound).all()
    dots_ok(dots, Ro, Xo, "unaligned")
    assert torch.equal(Xo, X)


def test_argument_errors(lz, handle, torch_cuda):
    torch = torch_cuda
    A, Ad, _, _ = operator(lz, "n49", F64)
    n, b = A.n, 16
    _, _, X, theta = inputs(torch, A, b, F64)
    R, dots = torch.zeros_like(X), nan_dots(torch, 1, b)
    big = torch.zeros(2 * n * b, dtype=torch.float64, device="cuda")
    cases = [
        ("R is X", dict(X=X, theta=theta, R=X, dots=dots)),
        ("R overlaps X", dict(X=big[:n * b].view(n, b), theta=theta, R=big[8:8 + n * b].view(n, b), dots=dots)),
        ("theta overlaps R", dict(X=X, theta=R.view(-1)[32:32 + b], R=R, dots=dots)),
        ("dots overlaps R", dict(X=X, theta=theta, R=R, dots=R.view(-1)[:2 * b])),
        ("dots overlaps X", dict(X=X, theta=theta, R=R, dots=X.view(-1)[:2 * b])),
        ("dots overlaps theta", dict(X=X, theta=big[:b], R=R, dots=big[8:8 + 2 * b])),
    ]
    for what, kw in cases:
        with pytest.raises(lz.LanczosError, match="status -1"):
            handle.spmm_resid(Ad, kw["X"], kw["theta"], kw["R"], dots=kw["dots"])
    # NULLs, at the C entry
    L, p = lz.hip_lib(), lambda t: None if t is None else t.data_ptr()
    head = (handle.ptr, n, A.nnz, p(Ad.row_ptr), p(Ad.col), p(Ad.val), Ad.dtype, b)
    for th_, x_, r_, d_ in [(None, X, R, dots), (theta, None, R, dots), (theta, X, None, dots), (theta, X, R, None)]:
        assert L.lz_csr_spmm_resid(*head, p(th_), p(x_), p(r_), p(d_)) == -1
    assert L.lz_csr_spmm_resid(None, *head[1:], p(theta), p(X), p(R), p(dots)) != 0
    # the wrapper's own checks
    for th_ in (theta.float(), theta[:b - 1], theta.cpu()):
        with pytest.raises(lz.LanczosError, match="theta is a contiguous fp64 device tensor"):
            handle.spmm_resid(Ad, X, th_, R)
    assert torch.equal(X, inputs(torch, A, b, F64)[2])
