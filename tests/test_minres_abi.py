"""The MINRES entry points are declared in lz_hip.h / lz_host.h, exported by the libraries and
bound (CPU-only: no compute calls); the Python constants are those of the C++ sources."""
import inspect
import os
import re

from test_cg_abi import declared_in, exported_by

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lz_minres_update", "lz_minres_solve"]
NEW_HOST = ["lzh_minres_start", "lzh_minres_scalars"]


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


def test_solve_takes_cg_solves_arguments(lz):
    args = {n: a for n, _, a in lz.HIP_SYMBOLS}
    assert args["lz_minres_solve"] == args["lz_cg_solve"]
    assert len(args["lz_minres_update"]) == 12
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lz_hip.h")).read(), flags=re.S)
    proto = lambda name: re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert norm(proto("lz_minres_solve")) == norm(proto("lz_cg_solve"))


def test_minres_constants(lz):
    txt = open(os.path.join(lz.PKG_DIR, "csrc", "lz_internal.hpp")).read()
    assert lz.MINRES_WORK_BLOCKS == 5 == int(re.search(r"\bkMinresWorkBlocks\s*=\s*(\d+)", txt).group(1))
    hpp = open(os.path.join(lz.PKG_DIR, "csrc", "lz_minres.hpp")).read()
    val = lambda name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", hpp).group(1))
    assert lz.MINRES_COEFS == 7 == val("kMinresCoefs")
    assert lz.MINRES_BREAKDOWN == 2 == val("kMinresBreakdown") == lz.CG_NOT_PD
    hdr = open(os.path.join(ROOT, "include", "lz_hip.h")).read()
    assert re.search(r"#define\s+LZ_MINRES_BREAKDOWN\s+2\b", hdr)


def test_handle_methods(lz):
    assert callable(lz.Handle.minres_update)
    assert list(inspect.signature(lz.Handle.minres_update).parameters) == ["self", "coef", "W", "U", "Uo", "D1", "D2",
                                                                           "X", "uu"]
    doc = lz.Handle.solve.__doc__
    assert 'method="minres"' in doc and "breakdown" in doc
