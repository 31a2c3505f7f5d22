"""The Chebyshev preconditioner's entry points are declared, exported and bound, its struct has the
header's layout, and the argument errors that need no device are refused (CPU-only: no compute
calls)."""
import ctypes
import inspect

import numpy as np
import pytest

from test_abi import declared, exported

HIP_NAMES = ["lz_csr_spmm_axpby4_dots", "lz_cgz_update", "lz_cheb_precond_apply", "lz_pcg_cheb_solve"]
HOST_NAMES = ["lzh_cheb_precond_coeffs", "lzh_cheb_precond_lo"]


def test_entry_points_are_declared_exported_and_bound(lz):
    syms, L = exported(lz.HIP_LIB), lz.hip_lib()
    bound = {n: args for n, _, args in lz.HIP_SYMBOLS}
    decl = declared("lz_hip.h", "lz_")
    for n in HIP_NAMES:
        assert n in decl and n in syms and hasattr(L, n) and n in bound
    # lz_csr_spmm_axpby4's arguments and dots; lz_cg_update's and Z; lz_cg_solve's and the preconditioner
    assert len(bound["lz_csr_spmm_axpby4_dots"]) == len(bound["lz_csr_spmm_axpby4"]) + 1 == 17
    assert len(bound["lz_cgz_update"]) == len(bound["lz_cg_update"]) + 1 == 12
    assert len(bound["lz_pcg_cheb_solve"]) == len(bound["lz_cg_solve"]) + 1 == 19
    assert len(bound["lz_cheb_precond_apply"]) == 14


def test_host_entry_points(lz):
    syms, H = exported(lz.HOST_LIB), lz.host_lib()
    bound = {n: (res, args) for n, res, args in lz.HOST_SYMBOLS}
    decl = declared("lz_host.h", "lzh_")
    for n in HOST_NAMES:
        assert n in decl and n in syms and hasattr(H, n) and n in bound
    assert bound["lzh_cheb_precond_lo"][0] is ctypes.c_double and len(bound["lzh_cheb_precond_coeffs"][1]) == 4


def test_struct_layout(lz):
    """typedef struct { int degree; double lo, hi; } lz_cheb_precond: 24 bytes, the doubles on 8."""
    S = lz.ChebPrecondSpec
    assert ctypes.sizeof(S) == 24
    assert (S.degree.offset, S.lo.offset, S.hi.offset) == (0, 8, 16)
    assert ctypes.sizeof(lz.Inverse) == 40  # untouched: the preconditioner is not an inner method of it


def test_constants_and_methods(lz):
    assert lz.CHEB_PCG_WORK_BLOCKS == 7 and lz.PCG_WORK_BLOCKS == 5 and lz.CHEB_PRECOND_MAX_DEGREE == 64
    for m in ("spmm_axpby4_dots", "cgz_update", "cheb_precond_apply", "solve"):
        assert callable(getattr(lz.Handle, m))
    assert inspect.signature(lz.Handle.solve).parameters["precond"].default is None
    p = lz.ChebPrecond()
    assert (p.degree, p.lo, p.hi) == (8, None, None)
    assert lz.ChebPrecond(3, 0.1, 8.0) == lz.ChebPrecond(degree=3, lo=0.1, hi=8.0)


@pytest.mark.parametrize("pc", [(0, 1.0, 2.0), (65, 1.0, 2.0), (1.5, 1.0, 2.0), (3, 0.0, 2.0), (3, 2.0, 2.0),
                                (3, 1.0, float("inf")), (3, float("nan"), 2.0), (3, None, 2.0)])
def test_python_refuses_bad_preconditioners(lz, pc):
    with pytest.raises(lz.LanczosError):
        lz._cheb_precond(pc)
    with pytest.raises(lz.LanczosError):
        lz._cheb_precond(lz.ChebPrecond(*pc))


def test_null_handle_is_refused(lz):
    """Every new entry point checks its handle first: a NULL handle is an error, never a crash."""
    L = lz.hip_lib()
    pc = lz.ChebPrecondSpec(3, 0.1, 8.0)
    z = np.zeros(4)
    assert L.lz_csr_spmm_axpby4_dots(None, 1, 1, None, None, None, lz.LZ_F64, 1, 1.0, None, 0.0, 0.0, None, 1.0, None,
                                     None, None) != 0
    assert L.lz_cgz_update(None, 1, 1, lz.LZ_F64, None, None, None, None, None, None, None, None) != 0
    assert L.lz_cheb_precond_apply(None, 1, 1, None, None, None, lz.LZ_F64, 1, 0.0, ctypes.addressof(pc), None, None,
                                   None, None) != 0
    opts = lz.CgOpts(1e-10, 10, 0, 3)
    assert L.lz_pcg_cheb_solve(None, 1, 1, None, None, None, lz.LZ_F64, 1, 0.0, ctypes.addressof(pc), None, None, None,
                               ctypes.addressof(opts), lz._p(z), lz._p(z), lz._p(z), lz._p(z), lz._p(z)) != 0
    assert b"handle" in L.lz_last_error()
