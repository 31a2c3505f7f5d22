"""Results must not depend on what a handle ran before.

lz_handle keeps about twenty workspaces between calls (lz_common.hpp), grown and never cleared;
every solve is meant to derive its plan, columns, row orders and flags anew.  These tests state
that contract over the catalogue of history_calls.py:

    test_call_matches_reference   each call on a handle of its own against its CPU reference, so
                                  that "the same bits" below cannot mean "equally wrong"
    test_call_reproducible        two handles of their own: the same bits (NaN positions included)
    test_after                    after every catalogue entry on the same handle (itself included):
                                  the bits of the handle of its own
    test_operator_replaced        the operator's three arrays overwritten in place by another of
                                  equal n and nnz: the bits of a new operator on a new handle
    test_two_handles_alternate    a wavefront solve and a CG solve on two handles, strictly one
                                  after the other: the process-wide statics

No test here shares the session's handle with a call under test, and none runs two handles'
launches at once: the wavefront step needs every block resident ("Co-residency").
"""
import numpy as np
import pytest

import history_calls as hc
from test_cg_host import gersh_shift
from test_gpu_wf_plan import plan_ref

pytestmark = pytest.mark.gpu

COMPARED = [n for n in hc.NAMES if n not in hc.NOT_REPRODUCIBLE]


@pytest.mark.parametrize("name", hc.NAMES)
def test_call_matches_reference(lz, torch_cuda, name):
    c, probe = hc.call(name), {}
    out = hc.run_fresh(name, probe)
    c.check(out, hc.inputs(name))
    if c.path is not None:
        c.path(probe, hc.inputs(name))
    if name in COMPARED:  # (a run that recorded its launches: the same bits as one that did not)
        assert hc.first_difference(out, hc.fresh(name)) is None


@pytest.mark.parametrize("name", hc.NAMES)
def test_call_reproducible(lz, torch_cuda, name):
    """DESIGN.md's claim for every family: static tile assignment, fixed-order folds, integer
    atomics only.  A call that fails here is recorded there and listed in NOT_REPRODUCIBLE."""
    diff = hc.first_difference(hc.run_fresh(name), hc.fresh(name))
    assert (diff is None) == (name in COMPARED), f"{name} on two handles of their own: {diff}"


@pytest.mark.parametrize("successor", COMPARED)
def test_after(lz, torch_cuda, successor):
    """Every predecessor, then the successor on new input tensors, on one handle."""
    want, c = hc.fresh(successor), hc.call(successor)
    found = []
    for p in hc.NAMES:
        h = lz.Handle(0)
        try:
            hc.call(p).run(h, hc.inputs(p))
            diff = hc.first_difference(c.run(h, hc.inputs(successor)), want)
        finally:
            h.close()
        if diff is not None:
            found.append(f"after {p}: {diff}")
    assert not found, f"{successor} depends on the handle's history:\n  " + "\n  ".join(found)


# ------------------------------------------------------------------ an operator replaced in place
def moved_far(lz, A, far=40_000):
    """A with eight symmetric off-diagonal pairs moved `far` columns away: for each of four rows
    r (and r' = r + far) with first off-diagonal neighbours c > r and c' > r', the entries (r, c),
    (c, r), (r', c'), (c', r') become (r, c'), (c, r'), (r', c), (c', r).  One replacement in each
    of the sixteen rows, the columns of a row sorted again, n and nnz unchanged, A still symmetric."""
    rp, col, val = A.row_ptr, A.col.copy(), A.val.copy()

    def neighbour(r):
        ks = np.arange(rp[r], rp[r + 1])
        return int(col[ks[col[ks] > r][0]])

    def replace(r, old, new, v):
        ks = np.arange(rp[r], rp[r + 1])
        k = ks[col[ks] == old][0]
        assert new not in col[ks]
        col[k], val[k] = new, v
        order = np.argsort(col[ks], kind="stable")
        col[ks], val[ks] = col[ks][order], val[ks][order]

    for i in range(4):
        r = 5000 * i + 123
        r2 = r + far
        c, c2 = neighbour(r), neighbour(r2)
        ks = np.arange(rp[r], rp[r + 1])
        v = float(val[ks[col[ks] == c][0]])
        replace(r, c, c2, v)
        replace(c2, r2, r, v)
        replace(c, r, r2, v)
        replace(r2, c2, c, v)
    return lz.CsrHost(A.n, rp.copy(), col, val)


_pairs = {}


def pair(lz, which):
    """(A1, A2): equal n and nnz, different structure."""
    if which not in _pairs:
        if which == "laplace":
            A1, A2 = lz.gen_laplace2d(40, 36), lz.gen_laplace2d(36, 40)
            assert (A1.n, A1.nnz) == (A2.n, A2.nnz) == (1440, 7048)
        else:
            A1 = lz.gen_banded(60_013, 10.0, 64, seed=11)
            A2 = moved_far(lz, A1)
            import scipy.sparse as sp
            M = sp.csr_matrix((A2.val, A2.col, A2.row_ptr), shape=(A2.n, A2.n))
            same_row = np.diff(np.repeat(np.arange(A2.n), np.diff(A2.row_ptr))) == 0
            assert abs(M - M.T).max() == 0 and (np.diff(A2.col)[same_row] > 0).all(), "A2: symmetric, rows sorted"
            assert int((A1.col != A2.col).sum()) >= 16
            # the wavefront plan must change its column form and its dependency ranges
            d1, _, _, bad1 = plan_ref(A1, 176)
            d2, _, _, bad2 = plan_ref(A2, 176)
            assert not bad1 and bad2 and not np.array_equal(d1, d2)
        assert (A1.n, A1.nnz) == (A2.n, A2.nnz) and not np.array_equal(A1.col, A2.col)
        _pairs[which] = (A1, A2)
    return _pairs[which]


def _block(env):
    def entry(lz, h, Ad, A):
        return hc.core_block(h, Ad, lz.uniform_B(A.n, 16, seed=5), 4, A.n // 3, True, env)
    return entry


def _spmm(env):
    def entry(lz, h, Ad, A):
        out = hc.core_spmm(h, Ad, np.random.default_rng(7).uniform(-1, 1, (A.n, 16)), env)
        if env:
            # The banded pair runs k_spmm_fnz.  The Laplacians do not: at 4.9 entries per row a tile of 448
            # entries owns 91 rows, more than the kernel's 88, so fnz_prepare refuses and the default kernel
            # runs (which is why that pair never showed the stale format)
            assert (int(out["kernel"]) == lz.LZ_K_FNZ) == (A.n > 1440), hex(int(out["kernel"]))
        return out
    return entry


ENTRIES = {
    "spmm": _spmm({}),
    "spmm-fnz": _spmm({"LZ_SPMM_FNZ": "1"}),
    "blk-wavefront": _block({}),
    "blk-twopass": _block({"LZ_PASS_WF": "0"}),
    "vector-lanczos": lambda lz, h, Ad, A: hc.core_vector(h, Ad, lz.uniform_B(A.n, 1, seed=3)[:, 0].copy(), 6, 84),
    "solve-jacobi": lambda lz, h, Ad, A: hc.core_solve(h, Ad, hc.rhs(A.n, 16, np.float64), shift=gersh_shift(lz, A),
                                                       precond="jacobi"),
    "eigsh": lambda lz, h, Ad, A: hc.core_eigsh(h, Ad, lz.uniform_B(A.n, 16), 16, b=16, m=6, keep=2, max_cycles=2),
    "transpose": lambda lz, h, Ad, A: hc.core_transpose(h, Ad),
}


@pytest.mark.parametrize("which", ["laplace", "banded-moved"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_operator_replaced(lz, torch_cuda, entry, which):
    """Every call reads the operator arrays it is given; nothing is kept across calls by address."""
    A1, A2 = pair(lz, which)
    run = ENTRIES[entry]
    h = lz.Handle(0)
    try:
        Ad = lz.CsrDevice.from_host(A1)
        ptrs = [t.data_ptr() for t in (Ad.row_ptr, Ad.col, Ad.val)]
        first = run(lz, h, Ad, A1)
        for t, a in ((Ad.row_ptr, A2.row_ptr), (Ad.col, A2.col), (Ad.val, A2.val)):
            t.copy_(torch_cuda.from_numpy(a))
        assert [t.data_ptr() for t in (Ad.row_ptr, Ad.col, Ad.val)] == ptrs
        got = run(lz, h, Ad, A2)
    finally:
        h.close()
    h2 = lz.Handle(0)
    try:
        want = run(lz, h2, lz.CsrDevice.from_host(A2), A2)
    finally:
        h2.close()
    assert hc.first_difference(first, want) is not None, "A1 and A2 give different results (the case can fail)"
    diff = hc.first_difference(got, want)
    assert diff is None, f"{entry} on A2 behind A1's addresses: {diff}"


# ------------------------------------------------------------------ two handles, one process
def test_two_handles_alternate(lz, torch_cuda):
    """Handle A runs the wavefront solve, handle B the CG solve, three rounds, a device
    synchronisation after every call (the two handles' launches never overlap): each result is
    the bits of a handle of its own.  Covers what the process keeps outside a handle: the
    occupancy cache of wf_step16 and the last-error text."""
    wf, cg = "blk-wf-col16", "solve-columns"
    ha, hb = lz.Handle(0), lz.Handle(0)
    try:
        for rnd in range(3):
            for h, name in ((ha, wf), (hb, cg)):
                out = hc.call(name).run(h, hc.inputs(name))  # (run synchronises the device before it returns)
                torch_cuda.cuda.synchronize()
                diff = hc.first_difference(out, hc.fresh(name))
                assert diff is None, f"round {rnd}, {name}: {diff}"
    finally:
        ha.close()
        hb.close()
