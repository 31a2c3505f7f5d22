"""The block conjugate-gradient entry points are declared in lz_hip.h / lz_host.h, exported by the
libraries and bound (CPU-only: no compute calls); the Python constants the GPU tests place their
edges by are those of csrc/lz_internal.hpp and csrc/lz_bcg.hpp."""
import os
import re

from test_cg_abi import declared_in, exported_by

NEW = ["lz_bcg_update", "lz_bcg_direction", "lz_bcg_solve"]
NEW_HOST = ["lzh_bcg_start", "lzh_bcg_start_finish", "lzh_bcg_mid", "lzh_bcg_end", "lzh_bcg_guard"]


def test_new_entry_points(lz):
    declared, exported = declared_in("lz_hip.h", "lz"), exported_by(lz.HIP_LIB)
    bound = {n for n, _, _ in lz.HIP_SYMBOLS}
    L = lz.hip_lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in lz_hip.h"
        assert name in exported, f"{name} not exported by liblz_hip.so"
        assert name in bound and hasattr(L, name), f"{name} not bound in HIP_SYMBOLS"


def test_new_host_entry_points(lz):
    declared, exported = declared_in("lz_host.h", "lzh"), exported_by(lz.HOST_LIB)
    bound = {n for n, _, _ in lz.HOST_SYMBOLS}
    L = lz.host_lib()
    for name in NEW_HOST:
        assert name in declared, f"{name} not declared in lz_host.h"
        assert name in exported, f"{name} not exported by liblz_host.so"
        assert name in bound and hasattr(L, name), f"{name} not bound in HOST_SYMBOLS"


def test_bcg_constants(lz):
    txt = open(os.path.join(lz.PKG_DIR, "csrc", "lz_internal.hpp")).read()
    val = lambda name, t=txt: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", t).group(1))
    assert lz.BCG_THREADS == val("kBcgThreads")
    assert lz.BCG_ROWS_16 == val("kBcgRows16") == 16 * lz.BCG_THREADS // 64
    assert lz.BCG_ROWS_32 == val("kBcgRows32") == 32 * lz.BCG_THREADS // 64
    assert lz.BCG_ROWS_GEN == val("kBcgRowsGen")
    hdr = open(os.path.join(os.path.dirname(lz.PKG_DIR), "include", "lz_hip.h")).read()
    for name in ("LZ_K_BCG16", "LZ_K_BCG32F", "LZ_K_BCG_GEN"):
        assert val(name, hdr) == getattr(lz, name)
    assert lz.BCG_GRID_CAP == val("kBcgGridCap")
    hpp = open(os.path.join(lz.PKG_DIR, "csrc", "lz_bcg.hpp")).read()
    assert lz.BCG_MAX_B == val("kBcgMaxB", hpp)
    for name, v in (("kBcgNone", lz.BCG_NONE), ("kBcgConverged", lz.BCG_CONVERGED), ("kBcgSpent", lz.BCG_SPENT),
                    ("kBcgRank", lz.BCG_RANK), ("kBcgNotPd", lz.BCG_NOT_PD)):
        assert val(name, hpp) == v


def test_solve_signature(lz):
    import inspect
    sig = inspect.signature(lz.Handle.solve)
    assert sig.parameters["method"].default == "columns"
    assert hasattr(lz.Handle, "bcg_update") and hasattr(lz.Handle, "bcg_direction")
