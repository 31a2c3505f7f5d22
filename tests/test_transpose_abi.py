"""The transpose and normal-operator entry points are declared in lz_hip.h, exported by
liblz_hip.so and bound in HIP_SYMBOLS (CPU-only: no compute calls)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lz_csr_transpose", "lz_normal_apply", "lz_block_lanczos_reorth_normal",
       "lz_block_lanczos_reorth_resume_normal"]


def test_new_entry_points(lz):
    txt = open(os.path.join(ROOT, "include", "lz_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lz_\w+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", lz.HIP_LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    bound = {n for n, _, _ in lz.HIP_SYMBOLS}
    L = lz.hip_lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in lz_hip.h"
        assert name in exported, f"{name} not exported by liblz_hip.so"
        assert name in bound and hasattr(L, name), f"{name} not bound in HIP_SYMBOLS"


def test_transpose_constants(lz):
    """The sort-class and scan-block sizes the GPU tests place their boundary cases at are those
    of csrc/lz_internal.hpp."""
    txt = open(os.path.join(lz.PKG_DIR, "csrc", "lz_internal.hpp")).read()
    val = lambda name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", txt).group(1))
    assert lz.TRANSPOSE_SHORT == val("kTrShort")
    assert lz.TRANSPOSE_LDS == val("kTrLds")
    assert lz.TRANSPOSE_SCAN_BLOCK == val("kTrScanThreads") * val("kTrScanPer")
