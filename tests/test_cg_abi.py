"""The conjugate-gradient entry points are declared in lz_hip.h / lz_host.h, exported by the
libraries and bound (CPU-only: no compute calls); the Python constants the GPU tests place
their edges by are those of csrc/lz_internal.hpp."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lz_cg_solve", "lz_cg_update"]
NEW_HOST = ["lzh_cg_start", "lzh_cg_scalars"]


def declared_in(header, prefix):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(" + prefix + r"_\w+)\s*\(", txt))


def exported_by(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


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


def test_cg_constants(lz):
    txt = open(os.path.join(lz.PKG_DIR, "csrc", "lz_internal.hpp")).read()
    val = lambda name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", txt).group(1))
    assert lz.CG_THREADS == val("kCgThreads")
    assert lz.CG_ROWS_128 == val("kCgRows128")
    assert lz.CG_GRID_CAP == val("kCgGridCap")
    assert lz.CG_CHECK_EVERY == val("kCgCheckEvery")
    hpp = open(os.path.join(lz.PKG_DIR, "csrc", "lz_cg.hpp")).read()
    for name, v in (("kCgMet", lz.CG_MET), ("kCgSpent", lz.CG_SPENT), ("kCgNotPd", lz.CG_NOT_PD)):
        assert int(re.search(r"\b" + name + r"\s*=\s*(\d+)", hpp).group(1)) == v


def test_opts_layout(lz):
    """CgOpts mirrors lz_cg_opts: {double tol; int max_iter, check_every, max_restarts;}."""
    import ctypes
    assert ctypes.sizeof(lz.CgOpts) == 24
    assert [f[0] for f in lz.CgOpts._fields_] == ["tol", "max_iter", "check_every", "max_restarts"]
    txt = open(os.path.join(ROOT, "include", "lz_hip.h")).read()
    assert re.search(r"double tol;\s*int max_iter, check_every, max_restarts;\s*}\s*lz_cg_opts;", txt)
