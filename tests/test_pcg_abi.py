"""The preconditioned solve's entry points are exported and bound (CPU-only: no compute calls)."""
from test_abi import exported


def test_pcg_entry_points_are_bound(lz):
    names = ["lz_pcg_update", "lz_csr_jacobi", "lz_pcg_solve"]
    syms = exported(lz.HIP_LIB)
    L = lz.hip_lib()
    bound = {n: args for n, _, args in lz.HIP_SYMBOLS}
    for n in names:
        assert n in syms and hasattr(L, n) and n in bound
    assert len(bound["lz_pcg_update"]) == 13 and len(bound["lz_csr_jacobi"]) == 10
    # lz_cg_solve's arguments and dinv
    assert len(bound["lz_pcg_solve"]) == len(bound["lz_cg_solve"]) + 1 == 19


def test_pcg_scalars_is_bound(lz):
    assert "lzh_pcg_scalars" in exported(lz.HOST_LIB) and hasattr(lz.host_lib(), "lzh_pcg_scalars")
    bound = {n: args for n, _, args in lz.HOST_SYMBOLS}
    # lzh_cg_scalars' arguments and rr
    assert len(bound["lzh_pcg_scalars"]) == len(bound["lzh_cg_scalars"]) + 1


def test_constants_and_methods(lz):
    assert lz.PCG_WORK_BLOCKS == 5
    assert lz.JACOBI_LANES * lz.JACOBI_ROWS == lz.CG_THREADS
    for m in ("jacobi", "pcg_update", "solve"):
        assert callable(getattr(lz.Handle, m))
    import inspect
    assert inspect.signature(lz.Handle.solve).parameters["precond"].default is None
