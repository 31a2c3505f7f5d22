"""The multi-shift conjugate-gradient entry points are declared in lz_hip.h / lz_host.h, exported
by the libraries and bound (CPU-only: no compute calls); MSCG_MAX_SHIFTS is csrc/lz_mscg.hpp's."""
import os
import re

from test_cg_abi import declared_in, exported_by

NEW = ["lz_mscg_update", "lz_mscg_solve"]
NEW_HOST = ["lzh_mscg_start", "lzh_mscg_scalars"]


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


def test_bound_argument_counts(lz):
    """The bindings carry as many arguments as the headers declare."""
    for header, table in (("lz_hip.h", lz.HIP_SYMBOLS), ("lz_host.h", lz.HOST_SYMBOLS)):
        txt = open(os.path.join(os.path.dirname(lz.PKG_DIR), "include", header)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for name, _, args in table:
            if "mscg" not in name:
                continue
            decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt).group(1)
            assert len(decl.split(",")) == len(args), name


def test_mscg_constants(lz):
    txt = open(os.path.join(lz.PKG_DIR, "csrc", "lz_mscg.hpp")).read()
    assert lz.MSCG_MAX_SHIFTS == int(re.search(r"\bkMscgMaxShifts\s*=\s*(\d+)", txt).group(1))
    assert hasattr(lz.Handle, "solve_shifts") and hasattr(lz.Handle, "mscg_update")
