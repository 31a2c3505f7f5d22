"""MI355X (gfx950) single- and block-Lanczos -- Python host mirror of the C ABI.

The product is two in-tree shared libraries built by ``make`` in this directory:

* ``lib/liblz_hip.so``  -- the gfx950 kernels and the Lanczos iteration behind the
  extern "C" boundary declared in ``include/lz_hip.h``;
* ``lib/liblz_host.so`` -- host logic (generators, formats, post-processing) from
  ``include/lz_host.h``.

This module binds both with ctypes and mirrors the reference's operator API
(ibrohimmn1994/GPU-implementation-of-signle-and-block-Lanczos, paths relative to
``source/``): ``spmm`` / ``spmv`` (kernels/spmv_spmm.hpp:209-333),
``mm_tt`` / ``mm_tt2`` / ``mm_ts`` (utils/lib_utils.hpp:28-202), ``sqrtm``
(lib_utils.hpp:721-745), ``block_lanczos_blas`` (methods/block_lanczos.hpp:88-167),
``vector_lanczos`` (methods/vector_lanczos.hpp:8-67), ``ftdt_block``
(methods/fdtd.hpp:33-56), ``Assemble_T`` + Ritz values + ``solution``
(test_lanczos.cu:272-286).  Device memory, streams and torch.distributed come
from PyTorch (plumbing only); every computation runs in liblz_hip.so.  There is
no CPU fallback: a GPU entry point raises if the HIP library cannot be loaded or
no gfx950 device is present.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
# LZ_HIP_LIB: another build of the same library (A/B of kernel versions in scripts/)
HIP_LIB = os.environ.get("LZ_HIP_LIB") or os.path.join(LIB_DIR, "liblz_hip.so")
HOST_LIB = os.path.join(LIB_DIR, "liblz_host.so")

LZ_F64, LZ_F32 = 0, 1
LZ_ROW_MAJOR, LZ_COL_MAJOR = 0, 1
# lz_debug_last_kernel ids (include/lz_hip.h): SpMM kernels, their flags, dense kernels
(LZ_K_SEG768, LZ_K_SEG1536, LZ_K_SEG1024, LZ_K_FNZ, LZ_K_BUF, LZ_K_LDS, LZ_K_ANY_B, LZ_K_CM_DIRECT,
 LZ_K_SPMV) = range(1, 10)
LZ_K_WIN, LZ_K_YCM, LZ_K_EPI, LZ_K_AX3, LZ_K_DOT = 0x100, 0x200, 0x400, 0x800, 0x1000
LZ_K_AX4 = 0x2000
LZ_K_RESID = 0x4000  # lz_csr_spmm_resid's fused residual store
LZ_K_RSC = 0x8000  # lz_csr_spmm_rowscale's fused row-scaled store
LZ_K_GRAM16, LZ_K_GRAM32F, LZ_K_GRAM_GEN, LZ_K_TSMM16, LZ_K_TSMM32F, LZ_K_TSMM_GEN = range(1, 7)
LZ_K_PGRAM16, LZ_K_PGRAM_GEN, LZ_K_PAPPLY16, LZ_K_PAPPLY_GEN = range(7, 11)
# blocks per group of the panel Gram kernels (W is re-read once per group): b = 16 fp64 MFMA, generic
PANEL_GROUP_16, PANEL_GROUP_GEN = 16, 4
PANEL_MAX_BLOCKS = 64
LZ_K_PCOMP16, LZ_K_PCOMP_GEN = 11, 12
PANEL_MAX_KEEP = 16  # most output blocks of one panel_compress (LZ_PANEL_MAX_KEEP)
# lz_csr_transpose (csrc/lz_internal.hpp kTr*): an output row of up to TRANSPOSE_SHORT entries is
# sorted by one lane group, up to TRANSPOSE_LDS by one workgroup through LDS, a longer one in
# chunks of TRANSPOSE_LDS merged pairwise; the scan covers TRANSPOSE_SCAN_BLOCK counts per workgroup
TRANSPOSE_SHORT, TRANSPOSE_LDS, TRANSPOSE_SCAN_BLOCK = 16, 4096, 2048
# lz_cg_update (csrc/lz_internal.hpp kCg*): CG_THREADS threads per block; the 128-byte-row form covers
# CG_ROWS_128 rows per block pass, the generic form CG_THREADS // b; at most CG_GRID_CAP blocks (one
# slab each), then grid-stride.  CG_CHECK_EVERY: lz_cg_solve's default iterations between two reads
# of the live count
CG_THREADS, CG_ROWS_128, CG_GRID_CAP, CG_CHECK_EVERY = 256, 32, 2048, 8
CG_MET, CG_SPENT, CG_NOT_PD = 0, 1, 2  # Handle.solve's status per column
MSCG_MAX_SHIFTS = 16  # Handle.solve_shifts' most shifts (csrc/lz_mscg.hpp kMscgMaxShifts)
# lz_pcg_solve's work is PCG_WORK_BLOCKS blocks of n b elements; lz_csr_jacobi (csrc/lz_internal.hpp
# kJacobi*) gives a row JACOBI_LANES lanes, a workgroup pass JACOBI_ROWS rows
PCG_WORK_BLOCKS, JACOBI_LANES, JACOBI_ROWS = 5, 8, 32
# lz_pcg_cheb_solve's work is CHEB_PCG_WORK_BLOCKS blocks of n b elements, [R | W | P | S | Z | T0 | T1];
# CHEB_PRECOND_MAX_DEGREE: the Chebyshev preconditioner's highest degree (csrc/lz_internal.hpp kCheb*)
CHEB_PCG_WORK_BLOCKS, CHEB_PRECOND_MAX_DEGREE = 7, 64
# lz_pcg_cheb_jacobi_solve's work: [R | W | P | S | Z | T0 | T1 | Rs] (csrc/lz_internal.hpp kChebJacobiPcgWorkBlocks)
CHEB_JACOBI_PCG_WORK_BLOCKS = 8
# lz_minres_solve's work is MINRES_WORK_BLOCKS blocks of n b elements (csrc/lz_internal.hpp kMinresWorkBlocks);
# lz_minres_update's coef has MINRES_COEFS rows of b; MINRES_BREAKDOWN: its status 2 (LZ_MINRES_BREAKDOWN)
MINRES_WORK_BLOCKS, MINRES_COEFS, MINRES_BREAKDOWN = 5, 7, 2
# lz_bcg_update / lz_bcg_direction (csrc/lz_internal.hpp kBcg*): BCG_THREADS threads per block; the b = 16
# fp64 MFMA form covers BCG_ROWS_16 rows per block pass (16-row tiles), the b = 32 fp32 one BCG_ROWS_32
# (32-row tiles), the generic form BCG_ROWS_GEN; at
# most BCG_GRID_CAP blocks (one b x b slab each), then grid-stride.  BCG_MAX_B: lz_bcg_solve's widest block
BCG_THREADS, BCG_ROWS_16, BCG_ROWS_32, BCG_ROWS_GEN, BCG_GRID_CAP, BCG_MAX_B = 256, 64, 128, 16, 1024, 32
LZ_K_BCG16, LZ_K_BCG32F, LZ_K_BCG_GEN = 13, 14, 15  # lz_debug_last_kernel's dense ids of the two passes
# Handle.solve(method="block")'s stop reason (csrc/lz_bcg.hpp kBcg*)
BCG_NONE, BCG_CONVERGED, BCG_SPENT, BCG_RANK, BCG_NOT_PD = 0, 1, 2, 3, 4


# the thick-restart drivers' rank test: a fresh beta block whose rank ratio (rank_ratios)
# is below delta -- or not finite -- is refused as rank deficient.  Per precision of the solve, for the
# start block's beta_0 (sigma_min / sigma_max) and for the blocks of the steps (sigma_min / max|theta|):
# the geometric means of the smallest healthy and the largest deficient ratio measured on the device
RANK_DELTA_START_F64, RANK_DELTA_START_F32 = 1.4e-5, 1.0e-5
RANK_DELTA_STEP_F64, RANK_DELTA_STEP_F32 = 2.4e-11, 2.5e-7


def bcg_guard(b: int, eps: float) -> float:
    """The block solver's rank guard: lambda_min > bcg_guard * lambda_max (lzh_bcg_guard)."""
    return max(1e-10, 64.0 * b * eps)


_c_i64, _c_i32, _c_int, _c_dbl, _c_vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
_c_u32, _c_u64 = ctypes.c_uint32, ctypes.c_uint64


class LanczosError(RuntimeError):
    """Raised for a non-zero status from liblz_hip.so / liblz_host.so."""


# --------------------------------------------------------------- library load
_hip = None
_host = None

# (name, restype, argtypes) of every symbol in include/lz_hip.h
HIP_SYMBOLS = [
    ("lz_init", _c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    ("lz_finalize", _c_int, [_c_vp]),
    ("lz_set_stream", _c_int, [_c_vp, _c_vp]),
    ("lz_set_final_state", _c_int, [_c_vp, _c_int]),
    ("lz_last_error", ctypes.c_char_p, []),
    ("lz_version", ctypes.c_char_p, []),
    ("lz_device_ok", _c_int, [_c_int]),
    ("lz_device_error", _c_int, [_c_vp, ctypes.POINTER(_c_int)]),
    ("lz_debug_poison_lds", _c_int, [_c_vp, ctypes.c_uint32]),
    ("lz_debug_set_device_error", _c_int, [_c_vp, _c_int]),
    ("lz_debug_fail_next_setup", _c_int, [_c_vp, _c_int]),
    ("lz_prof_enable", _c_int, [_c_vp, _c_int]),
    ("lz_prof_enable_mask", _c_int, [_c_vp, ctypes.c_uint]),
    ("lz_prof_read", _c_int, [_c_vp, _c_int, ctypes.POINTER(_c_dbl), ctypes.POINTER(_c_int)]),
    ("lz_csr_spmm", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int,
                             _c_vp, _c_i64, _c_int, _c_vp, _c_i64]),
    ("lz_to_row_major", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_i64, _c_vp]),
    ("lz_to_col_major", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_i64]),
    ("lz_csr_spmv", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp]),
    ("lz_gram", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_i64, _c_vp]),
    ("lz_sym_cross_gram", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_i64, _c_vp]),
    ("lz_tsmm", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp, _c_i64]),
    ("lz_sqrtm_pair", _c_int, [_c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_copy_row", _c_int, [_c_vp, _c_int, _c_int, _c_vp, _c_i64, _c_int, _c_i64, _c_vp, _c_i64]),
    ("lz_block_lanczos", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                  _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_block_lanczos_unfused", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int,
                                          _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_panel_gram", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_int, _c_vp, _c_i64, _c_vp, _c_vp]),
    ("lz_panel_apply", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_int, _c_dbl, _c_dbl, _c_vp, _c_i64, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                         _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_int]),
    ("lz_panel_compress", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_i64, _c_vp]),
    ("lz_block_lanczos_reorth_resume", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                                _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp,
                                                _c_int]),
    ("lz_csr_spmm_axpby", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp,
                                   _c_dbl, _c_dbl, _c_vp, _c_vp]),
    ("lz_cheb_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                               _c_vp]),
    ("lz_col_dots", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lz_csr_spmm_axpby_dots", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp,
                                        _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp]),
    ("lz_csr_spmm_resid", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                                   _c_vp]),
    ("lz_cheb_moments", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_dbl, _c_int,
                                 _c_vp, _c_vp, _c_vp]),
    ("lz_cg_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_cg_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp, _c_vp,
                             _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_mscg_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp]),
    ("lz_mscg_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                               _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_pcg_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                               _c_vp]),
    ("lz_csr_jacobi", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_dbl, _c_vp, _c_vp]),
    ("lz_pcg_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp, _c_vp,
                              _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_csr_spmm_axpby4_dots", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp,
                                         _c_dbl, _c_dbl, _c_vp, _c_dbl, _c_vp, _c_vp, _c_vp]),
    ("lz_cgz_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_cheb_precond_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp,
                                       _c_vp, _c_vp, _c_vp]),
    ("lz_pcg_cheb_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp,
                                   _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_csr_spmm_rowscale", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_dbl, _c_dbl,
                                      _c_vp, _c_dbl, _c_vp, _c_dbl, _c_dbl, _c_vp, _c_vp, _c_vp]),
    ("lz_cgzs_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_vp]),
    ("lz_cheb_jacobi_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp,
                                      _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_pcg_cheb_jacobi_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp,
                                          _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_bcg_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_bcg_direction", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_bcg_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp, _c_vp,
                              _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_minres_update", _c_int, [_c_vp, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                  _c_vp]),
    ("lz_minres_solve", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp, _c_vp,
                                 _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_cheb", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                              _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_int,
                                              _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_resume_cheb", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int,
                                                     _c_int, _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                                     _c_i64, _c_vp, _c_int, _c_vp, _c_vp]),
    ("lz_csr_spmm_axpby4", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_dbl, _c_vp,
                                    _c_dbl, _c_dbl, _c_vp, _c_dbl, _c_vp, _c_vp]),
    ("lz_cheb_series_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_dbl,
                                      _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_series", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                                _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_int,
                                                _c_int, _c_dbl, _c_dbl, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_resume_series", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int,
                                                       _c_int, _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                                       _c_i64, _c_vp, _c_int, _c_int, _c_dbl, _c_dbl, _c_vp, _c_vp]),
    ("lz_csr_transpose", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lz_normal_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_int,
                                 _c_int, _c_vp, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_normal", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                                _c_vp, _c_int, _c_int, _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp,
                                                _c_vp, _c_i64, _c_vp, _c_int, _c_vp]),
    ("lz_block_lanczos_reorth_resume_normal", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp,
                                                       _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_i64, _c_vp,
                                                       _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_int, _c_vp]),
    ("lz_inverse_apply", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                                  _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_inverse", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                                 _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_int,
                                                 _c_vp, _c_vp, _c_vp]),
    ("lz_block_lanczos_reorth_resume_inverse", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int,
                                                        _c_int, _c_int, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                                        _c_i64, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lz_vector_lanczos", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_i64,
                                   _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_fdtd_block", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_vp,
                               _c_i64, _c_dbl, _c_i64, _c_vp, _c_vp, _c_vp]),
    ("lz_comm_unique_id", _c_int, [_c_vp]),
    ("lz_comm_init", _c_int, [_c_vp, _c_int, _c_int, _c_vp]),
    ("lz_halo_init", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp]),
    ("lz_halo_sizes", _c_int, [_c_vp, _c_vp, _c_vp]),
    ("lz_halo_exchange", _c_int, [_c_vp, _c_int, _c_int, _c_vp]),
    ("lz_block_lanczos_halo", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int,
                                       _c_i64, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lz_comm_destroy", _c_int, [_c_vp]),
    ("lz_local_group_create", _c_int, [_c_int, _c_int, ctypes.POINTER(_c_vp)]),
    ("lz_local_group_destroy", _c_int, [_c_vp]),
    ("lz_local_group_abort", _c_int, [_c_vp]),
    ("lz_comm_init_local", _c_int, [_c_vp, _c_vp, _c_int]),
    ("lz_comm_abort", _c_int, [_c_vp]),
    ("lz_debug_last_split", _c_int, [_c_vp, _c_vp]),
    ("lz_debug_last_wf", _c_int, [_c_vp, ctypes.POINTER(_c_int)]),
    ("lz_debug_last_kernel", _c_int, [_c_vp, ctypes.POINTER(_c_int)]),
    ("lz_debug_wf_plan", _c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp,
                                  ctypes.POINTER(_c_int)]),
    ("lz_block_lanczos_dist", _c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp,
                                       _c_int, _c_int, _c_int, _c_i64, _c_int, _c_vp, _c_vp, _c_vp,
                                       _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
]

HOST_SYMBOLS = [
    ("lzh_gen_banded_count", _c_i64, [_c_i64, _c_dbl, _c_i64, _c_u64, _c_vp]),
    ("lzh_gen_banded_fill", _c_int, [_c_i64, _c_dbl, _c_i64, _c_u64, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_gen_banded_local_count", _c_i64, [_c_i64, _c_dbl, _c_i64, _c_u64, _c_i64, _c_i64, _c_vp]),
    ("lzh_gen_banded_local_fill", _c_int, [_c_i64, _c_dbl, _c_i64, _c_u64, _c_i64, _c_i64, _c_vp, _c_vp,
                                           _c_vp, _c_vp]),
    ("lzh_gen_powerlaw_count", _c_i64, [_c_i64, _c_dbl, _c_dbl, _c_i64, _c_u64, _c_vp]),
    ("lzh_gen_powerlaw_fill", _c_int, [_c_i64, _c_dbl, _c_dbl, _c_i64, _c_u64, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_matrix_a_shape", _c_int, [_c_int, _c_vp, _c_vp]),
    ("lzh_matrix_a_ell", _c_int, [_c_int, _c_int, _c_vp, _c_vp]),
    ("lzh_ell_to_csr_count", _c_i64, [_c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp]),
    ("lzh_ell_to_csr_fill", _c_int, [_c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_rand_B", _c_int, [_c_i64, _c_int, _c_u32, _c_i64, _c_int, _c_vp]),
    ("lzh_rand_lc", _c_i64, [_c_u32]),
    ("lzh_uniform_B", _c_int, [_c_i64, _c_int, _c_u64, _c_vp, _c_vp]),
    ("lzh_uniform_B_rows", _c_int, [_c_i64, _c_i64, _c_int, _c_u64, _c_vp, _c_vp]),
    ("lzh_sym_eig", _c_int, [_c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_assemble_T", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_ritz_values", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_ritz_pairs", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_ritz_pairs_dense", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_restart_coeffs", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_restart_fill", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_ritz_pairs_dense_mag", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_restart_coeffs_mag", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_gershgorin", _c_int, [_c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_cg_start", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                              _c_vp]),
    ("lzh_cg_scalars", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                _c_vp, _c_vp]),
    ("lzh_pcg_scalars", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                 _c_vp, _c_vp, _c_vp]),
    ("lzh_mscg_start", _c_int, [_c_int, _c_int, _c_int] + [_c_vp] * 16),
    ("lzh_mscg_scalars", _c_int, [_c_int, _c_int, _c_int, _c_int] + [_c_vp] * 19),
    ("lzh_gershgorin_jacobi", _c_int, [_c_i64, _c_vp, _c_vp, _c_vp, _c_dbl, _c_vp]),
    ("lzh_cheb_precond_coeffs", _c_int, [_c_int, _c_dbl, _c_dbl, _c_vp]),
    ("lzh_cheb_precond_lo", _c_dbl, [_c_int, _c_dbl]),
    ("lzh_minres_start", _c_int, [_c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_minres_scalars", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_bcg_start", _c_int, [_c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_bcg_start_finish", _c_int, [_c_int, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_bcg_mid", _c_int, [_c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_bcg_end", _c_int, [_c_int, _c_int, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_bcg_guard", _c_dbl, [_c_int, _c_dbl]),
    ("lzh_kpm_moments", _c_int, [_c_int, _c_int, _c_vp, _c_vp]),
    ("lzh_jackson", _c_int, [_c_int, _c_vp]),
    ("lzh_kpm_count", _c_int, [_c_int, _c_vp, _c_vp, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_vp]),
    ("lzh_cheb_window", _c_int, [_c_int, _c_dbl, _c_dbl, _c_dbl, _c_dbl, _c_vp, _c_vp]),
    ("lzh_kpm_density", _c_int, [_c_int, _c_vp, _c_vp, _c_dbl, _c_dbl, _c_int, _c_vp, _c_vp]),
    ("lzh_block_solution", _c_int, [_c_int, _c_int, _c_dbl, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_partition_rows", _c_int, [_c_i64, _c_vp, _c_int, _c_vp]),
    ("lzh_remap_cols_padded", _c_int, [_c_i64, _c_vp, _c_int, _c_vp, _c_i64, _c_vp]),
    ("lzh_halo_plan", _c_i64, [_c_i64, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_vp, _c_vp]),
    ("lzh_csr_write", _c_int, [ctypes.c_char_p, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_int]),
    ("lzh_csr_read_header", _c_int, [ctypes.c_char_p, _c_vp, _c_vp, _c_vp, _c_vp]),
    ("lzh_csr_read", _c_int, [ctypes.c_char_p, _c_vp, _c_vp, _c_vp]),
    ("lzh_num_threads", _c_int, []),
]


def _bind(lib, symbols, strict=True):
    for name, res, args in symbols:
        if not strict and not hasattr(lib, name):
            continue  # (an older build loaded through LZ_HIP_LIB for an A/B: only what it has)
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def build(verbose: bool = False) -> None:
    """Compile liblz_hip.so (hipcc --offload-arch=gfx950), liblz_host.so and test_lanczos in-tree."""
    import subprocess
    jobs = str(min(16, os.cpu_count() or 4))
    out = subprocess.run(["make", "-C", PKG_DIR, "-j", jobs], capture_output=not verbose, text=True)
    if out.returncode != 0:
        raise LanczosError("build failed:\n" + (out.stdout or "") + (out.stderr or ""))


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise LanczosError(f"{HOST_LIB} missing: run make in {PKG_DIR}")
        _host = _bind(ctypes.CDLL(HOST_LIB), HOST_SYMBOLS)
    return _host


def hip_lib():
    """liblz_hip.so with every symbol of include/lz_hip.h bound (loads without a GPU)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise LanczosError(f"{HIP_LIB} missing: run make in {PKG_DIR}")
        # PyTorch bundles its own HIP runtime / RCCL under the same SONAMEs
        # (libamdhip64.so.7, librccl.so.1).  Import it first so the dynamic
        # loader resolves liblz_hip.so's dependencies to the copies already in
        # the process: one HIP runtime per process, shared with torch's
        # allocator and streams.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip = _bind(ctypes.CDLL(HIP_LIB), HIP_SYMBOLS, strict=not os.environ.get("LZ_HIP_LIB"))
    return _hip


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = hip_lib().lz_last_error().decode(errors="replace") if _hip is not None else ""
        raise LanczosError(f"{what} failed with status {rc}: {msg}")


def _p(a: np.ndarray):
    return a.ctypes.data_as(_c_vp)


# ============================================================ host helpers
@dataclass
class CsrHost:
    """CSR on the host: int64 row_ptr, int32 col, float64/float32 val."""
    n: int
    row_ptr: np.ndarray
    col: np.ndarray
    val: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.row_ptr[-1])


def gen_banded(n: int, nnz_per_row: float = 10.0, halfwidth: int = 4096, seed: int = 20261015,
               dtype=np.float64) -> CsrHost:
    """Symmetric banded-random CSR."""
    L = host_lib()
    rp = np.empty(n + 1, np.int64)
    nnz = L.lzh_gen_banded_count(n, nnz_per_row, halfwidth, seed, _p(rp))
    if nnz < 0:
        raise LanczosError("lzh_gen_banded_count failed")
    col = np.empty(nnz, np.int32)
    val = np.empty(nnz, dtype)
    v64 = _p(val) if dtype == np.float64 else None
    v32 = _p(val) if dtype == np.float32 else None
    if L.lzh_gen_banded_fill(n, nnz_per_row, halfwidth, seed, _p(rp), _p(col), v64, v32):
        raise LanczosError("lzh_gen_banded_fill failed")
    return CsrHost(n, rp, col, val)


def gen_banded_local(n: int, r0: int, r1: int, nnz_per_row: float = 10.0, halfwidth: int = 4096,
                     seed: int = 20261015, dtype=np.float64) -> CsrHost:
    """Rows [r0, r1) of gen_banded(n, ...) with global column indices (one rank's slab)."""
    L = host_lib()
    nl = r1 - r0
    rp = np.empty(nl + 1, np.int64)
    nnz = L.lzh_gen_banded_local_count(n, nnz_per_row, halfwidth, seed, r0, r1, _p(rp))
    if nnz < 0:
        raise LanczosError("lzh_gen_banded_local_count failed")
    col = np.empty(nnz, np.int32)
    val = np.empty(nnz, dtype)
    v64 = _p(val) if dtype == np.float64 else None
    v32 = _p(val) if dtype == np.float32 else None
    if L.lzh_gen_banded_local_fill(n, nnz_per_row, halfwidth, seed, r0, r1, _p(rp), _p(col), v64, v32):
        raise LanczosError("lzh_gen_banded_local_fill failed")
    return CsrHost(nl, rp, col, val)


def gen_powerlaw(n: int, nnz_per_row: float = 10.0, a: float = 2.1, cap: int = 100000,
                 seed: int = 20261015, dtype=np.float32) -> CsrHost:
    """Symmetric power-law-degree CSR (config C5)."""
    L = host_lib()
    rp = np.empty(n + 1, np.int64)
    nnz = L.lzh_gen_powerlaw_count(n, nnz_per_row, a, cap, seed, _p(rp))
    if nnz < 0:
        raise LanczosError("lzh_gen_powerlaw_count failed")
    col = np.empty(nnz, np.int32)
    val = np.empty(nnz, dtype)
    v64 = _p(val) if dtype == np.float64 else None
    v32 = _p(val) if dtype == np.float32 else None
    if L.lzh_gen_powerlaw_fill(n, nnz_per_row, a, cap, seed, _p(rp), _p(col), v64, v32):
        raise LanczosError("lzh_gen_powerlaw_fill failed")
    return CsrHost(n, rp, col, val)


def gen_laplace2d(nx: int, ny: int, dtype=np.float64) -> CsrHost:
    """The 5-point Laplacian of an nx x ny grid with Dirichlet boundaries (4 on the
    diagonal, -1 to each neighbour; row iy*nx + ix, columns sorted).  Its eigenvalues are
    4 - 2 cos(i pi / (nx+1)) - 2 cos(j pi / (ny+1)), inside the Gershgorin interval [0, 8]."""
    if nx < 1 or ny < 1:
        raise ValueError("gen_laplace2d: nx, ny >= 1")
    n = nx * ny
    i = np.arange(n, dtype=np.int64)
    ix, iy = i % nx, i // nx
    # the row's five slots in column order; absent neighbours masked out
    cols = np.stack([i - nx, i - 1, i, i + 1, i + nx], axis=1)
    mask = np.stack([iy > 0, ix > 0, np.ones(n, bool), ix < nx - 1, iy < ny - 1], axis=1)
    vals = np.broadcast_to(np.array([-1, -1, 4, -1, -1], dtype), (n, 5))
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=rp[1:])
    return CsrHost(n, rp, cols[mask].astype(np.int32), np.ascontiguousarray(vals[mask]))


def gershgorin(A: CsrHost):
    """(lo, hi): the Gershgorin enclosure of a square CSR operator's spectrum
    (lzh_gershgorin; fp64 whatever A's precision).  An empty row's disc is [0, 0]."""
    out = np.empty(2)
    host = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()  # (a CsrDevice: copied back once)
    val = np.ascontiguousarray(host(A.val), np.float64)
    if host_lib().lzh_gershgorin(A.n, _p(np.ascontiguousarray(host(A.row_ptr), np.int64)),
                                 _p(np.ascontiguousarray(host(A.col), np.int32)), _p(val), _p(out)):
        raise LanczosError("lzh_gershgorin failed (n >= 1)")
    return float(out[0]), float(out[1])


def gershgorin_jacobi(A: CsrHost, shift: float = 0.0):
    """(lo, hi): the Gershgorin enclosure of N = D^-1/2 (A + shift I) D^-1/2, D the diagonal of A +
    shift I (lzh_gershgorin_jacobi; fp64 whatever A's precision): N has a unit diagonal, so (1 - rad,
    1 + rad) with rad = max_i sum_{j != i} |a_ij| / sqrt(d_i d_j).  What ChebPrecond(jacobi=True)
    takes for hi.  Raises LanczosError when a d_i is not positive and finite."""
    out = np.empty(2)
    host = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()  # (a CsrDevice: copied back once)
    val = np.ascontiguousarray(host(A.val), np.float64)
    rc = host_lib().lzh_gershgorin_jacobi(A.n, _p(np.ascontiguousarray(host(A.row_ptr), np.int64)),
                                          _p(np.ascontiguousarray(host(A.col), np.int32)), _p(val), float(shift),
                                          _p(out))
    if rc == -2:
        raise LanczosError("gershgorin_jacobi: a row of A + shift I has a diagonal that is not positive and finite")
    if rc:
        raise LanczosError("lzh_gershgorin_jacobi failed (n >= 1, shift finite)")
    return float(out[0]), float(out[1])


def cheb_precond_lo(degree: int, hi: float) -> float:
    """The Chebyshev preconditioner's default lower end, hi / (4 (degree + 1)^2) (lzh_cheb_precond_lo)."""
    return float(host_lib().lzh_cheb_precond_lo(int(degree), float(hi)))


def cheb_precond_coeffs(degree: int, lo: float, hi: float) -> np.ndarray:
    """(degree, 4) fp64: row j - 1 = the (a, c, d, e) of step j of the Chebyshev polynomial
    preconditioner on [lo, hi] as lz_cheb_precond_apply applies it (lzh_cheb_precond_coeffs): step 1
    is a three-term step on r, step 2 has d = 0 (its z_1 = r / theta travels in e)."""
    out = np.empty((max(int(degree), 1), 4))
    if host_lib().lzh_cheb_precond_coeffs(int(degree), float(lo), float(hi), _p(out)):
        raise LanczosError("cheb_precond_coeffs: 1 <= degree <= 64 and 0 < lo < hi, finite")
    return out


def kpm_moments(dots: np.ndarray) -> np.ndarray:
    """(K+1, 2, b) raw dots of Handle.cheb_moments -> (2K+1, b) Chebyshev moments, column c those
    of probe c (lzh_kpm_moments: mu_2k = 2 <t_k,t_k> - mu_0, mu_2k+1 = 2 <t_k+1,t_k> - mu_1)."""
    dots = np.ascontiguousarray(dots, np.float64)
    if dots.ndim != 3 or dots.shape[1] != 2:
        raise LanczosError("kpm_moments: dots is (K+1, 2, b)")
    K, b = dots.shape[0] - 1, dots.shape[2]
    mu = np.empty((2 * K + 1, b))
    if host_lib().lzh_kpm_moments(K, b, _p(dots), _p(mu)):
        raise LanczosError("lzh_kpm_moments failed (K, b >= 1)")
    return mu


def jackson(M: int) -> np.ndarray:
    """The Jackson damping factors g_0 .. g_{M-1} of a series of M moments (lzh_jackson)."""
    g = np.empty(max(int(M), 0))
    if host_lib().lzh_jackson(int(M), _p(g)):
        raise LanczosError("lzh_jackson failed (M >= 1)")
    return g


def _damping(damping, M: int):
    if damping not in ("jackson", None):
        raise LanczosError('damping: "jackson" or None')
    return jackson(M) if damping == "jackson" else None


def kpm_count(mu: np.ndarray, lo: float, hi: float, a: float, b: float, damping="jackson") -> float:
    """The eigenvalue count of [a, b] from the moments mu[0 .. M) of one probe, or of their mean
    (lzh_kpm_count), on the enclosure [lo, hi] the moments were taken with."""
    mu = np.ascontiguousarray(mu, np.float64)
    g, out = _damping(damping, mu.size), np.empty(1)
    if mu.ndim != 1 or host_lib().lzh_kpm_count(mu.size, _p(mu), None if g is None else _p(g), lo, hi, a, b, _p(out)):
        raise LanczosError("lzh_kpm_count failed (M >= 1, lo < hi finite, a <= b)")
    return float(out[0])


def cheb_window(degree: int, lo: float, hi: float, a: float, b: float, damping="jackson") -> np.ndarray:
    """The degree + 1 Chebyshev coefficients of the indicator of the window [a, b] on the
    enclosure [lo, hi] (lzh_cheb_window): gamma_k = g_k times the weights kpm_count applies to
    the moments, so cheb_window(...) @ mu == kpm_count(mu, ...).  lo <= a <= b <= hi.
    Handle.cheb_series_apply evaluates the series on an operator."""
    M = int(degree) + 1
    if M < 1:
        raise LanczosError("cheb_window: degree >= 0")
    g, gamma = _damping(damping, M), np.empty(M)
    if host_lib().lzh_cheb_window(M, lo, hi, a, b, None if g is None else _p(g), _p(gamma)):
        raise LanczosError("lzh_cheb_window failed (lo < hi finite, lo <= a <= b <= hi)")
    return gamma


def kpm_density(mu: np.ndarray, lo: float, hi: float, x, damping="jackson") -> np.ndarray:
    """The density of states at the points x from the moments mu[0 .. M) (lzh_kpm_density);
    0 outside (lo, hi)."""
    mu = np.ascontiguousarray(mu, np.float64)
    x = np.ascontiguousarray(np.atleast_1d(x), np.float64)
    g, rho = _damping(damping, mu.size), np.empty(x.size)
    if mu.ndim != 1 or host_lib().lzh_kpm_density(mu.size, _p(mu), None if g is None else _p(g), lo, hi, x.size, _p(x),
                                                  _p(rho)):
        raise LanczosError("lzh_kpm_density failed (M >= 1, lo < hi finite)")
    return rho.reshape(x.shape)


class KpmMoments:
    """Chebyshev moments of a symmetric operator from random probes (Handle.spectral_moments):
    n, the enclosure [lo, hi], mu ((2K+1) x probes, column c the moments x_c^T T_k(Ah) x_c of
    probe c) and n_spmm.  Host only: one set of moments serves any number of intervals."""

    def __init__(self, n: int, lo: float, hi: float, mu: np.ndarray, n_spmm: int):
        self.n, self.lo, self.hi, self.n_spmm = int(n), float(lo), float(hi), int(n_spmm)
        self.mu = np.ascontiguousarray(mu, np.float64)

    @property
    def probes(self) -> int:
        return self.mu.shape[1]

    def _mean(self, per_probe: np.ndarray):
        """(mean, sample standard deviation / sqrt(probes)) over the probes (axis 0)."""
        p = per_probe.shape[0]
        sd = per_probe.std(axis=0, ddof=1) / np.sqrt(p) if p > 1 else np.full(per_probe.shape[1:], np.nan)
        return per_probe.mean(axis=0), sd

    def count(self, a: float, b: float, damping="jackson"):
        """(estimate, stderr) of the number of eigenvalues in [a, b]: the mean of the per-probe
        counts and their sample standard deviation / sqrt(probes).  The resolution is about
        pi (hi - lo) / (2 M) for M moments."""
        est, sd = self._mean(np.array([kpm_count(col, self.lo, self.hi, a, b, damping) for col in self.mu.T]))
        return float(est), float(sd)

    def density(self, x, damping="jackson"):
        """(rho, stderr) at the points x: eigenvalues per unit length, integrating to n."""
        return self._mean(np.stack([kpm_density(col, self.lo, self.hi, x, damping) for col in self.mu.T]))


class ChebFilter(ctypes.Structure):
    """lz_cheb (include/lz_hip.h): the scaled Chebyshev filter of `degree` that damps
    [lo, hi] and is 1 at ref."""
    _fields_ = [("degree", _c_int), ("lo", _c_dbl), ("hi", _c_dbl), ("ref", _c_dbl)]


class CgOpts(ctypes.Structure):
    """lz_cg_opts (include/lz_hip.h): check_every 0 = the library's default."""
    _fields_ = [("tol", _c_dbl), ("max_iter", _c_int), ("check_every", _c_int), ("max_restarts", _c_int)]


class ChebPrecondSpec(ctypes.Structure):
    """lz_cheb_precond (include/lz_hip.h): the Chebyshev polynomial preconditioner of `degree` on [lo, hi]."""
    _fields_ = [("degree", _c_int), ("lo", _c_dbl), ("hi", _c_dbl)]


@dataclass
class ChebPrecond:
    """Handle.solve(precond=ChebPrecond(...)): z = q(A + shift I) r, the Chebyshev semi-iteration's
    polynomial of `degree` SpMMs on [lo, hi].  hi None: the Gershgorin upper bound of A + shift I;
    lo None: hi / (4 (degree + 1)^2).  jacobi=True: the Jacobi-scaled form z = q(D^-1 M) D^-1 r, D the
    diagonal of M = A + shift I, for a diagonal that varies; [lo, hi] then encloses D^-1/2 M D^-1/2
    and hi None takes gershgorin_jacobi(A, shift)[1]."""
    degree: int = 8
    lo: Optional[float] = None
    hi: Optional[float] = None
    jacobi: bool = False


def _cheb_precond(pc) -> ChebPrecondSpec:
    """A ChebPrecondSpec from a ChebPrecond with both ends given or a (degree, lo, hi) tuple, checked."""
    degree, lo, hi = (pc.degree, pc.lo, pc.hi) if isinstance(pc, (ChebPrecond, ChebPrecondSpec)) else pc
    if lo is None or hi is None:
        raise LanczosError("Chebyshev preconditioner: lo and hi are needed here")
    if int(degree) != degree or not 1 <= degree <= CHEB_PRECOND_MAX_DEGREE:
        raise LanczosError(f"Chebyshev preconditioner: 1 <= degree <= {CHEB_PRECOND_MAX_DEGREE}")
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise LanczosError(f"Chebyshev preconditioner: 0 < lo < hi, finite (got {lo}, {hi})")
    return ChebPrecondSpec(int(degree), float(lo), float(hi))


class Inverse(ctypes.Structure):
    """lz_inverse (include/lz_hip.h): (A - sigma I)^-1 through an inner solve; method 0 MINRES,
    1 column CG, 2 block CG."""
    _fields_ = [("sigma", _c_dbl), ("method", _c_int), ("opts", CgOpts)]


class InverseInfo(ctypes.Structure):
    """lz_inverse_info (include/lz_hip.h): what the inner solves of an inverse operator did.
    Every call that takes one accumulates into it; a fresh one is zero."""
    _fields_ = [("solves", _c_i64), ("passes", _c_i64), ("n_spmm", _c_i64), ("not_met", _c_i64),
                ("breakdown", _c_i64), ("worst", _c_dbl)]


INNER_METHODS = {"minres": 0, "columns": 1, "block": 2}
# Handle.eigsh(sigma=...): the default inner tolerance is this multiple of tol (the
# largest power of ten at which the stand-in's cases keep the exact-solve cycle count), clipped
# from below at INNER_TOL_FLOOR_EPS * eps of the operator's dtype
INNER_TOL_FACTOR = 1.0
INNER_TOL_FLOOR_EPS = 64.0


def _cheb(filt):
    """A ChebFilter from a (degree, lo, hi, ref) tuple (or one passed through)."""
    if isinstance(filt, ChebFilter):
        return filt
    degree, lo, hi, ref = filt
    return ChebFilter(int(degree), float(lo), float(hi), float(ref))


def matrix_a_ell(N: int, bug_compat: bool = False):
    """The reference's Yee operator A = D*W as ELL (column-major slots, width 4)."""
    L = host_lib()
    n, s = _c_i64(), _c_i64()
    L.lzh_matrix_a_shape(N, ctypes.byref(n), ctypes.byref(s))
    d = np.empty(s.value, np.float64)
    ix = np.empty(s.value, np.uint32)
    if L.lzh_matrix_a_ell(N, int(bug_compat), _p(d), _p(ix)):
        raise LanczosError("lzh_matrix_a_ell failed")
    return n.value, d, ix


def ell_to_csr(n: int, width: int, data: np.ndarray, idx: np.ndarray, keep_zeros: bool = False) -> CsrHost:
    L = host_lib()
    data = np.ascontiguousarray(data, np.float64)
    idx = np.ascontiguousarray(idx, np.uint32)
    rp = np.empty(n + 1, np.int64)
    nnz = L.lzh_ell_to_csr_count(n, width, _p(data), _p(idx), int(keep_zeros), _p(rp))
    col = np.empty(nnz, np.int32)
    val = np.empty(nnz, np.float64)
    L.lzh_ell_to_csr_fill(n, width, _p(data), _p(idx), int(keep_zeros), _p(rp), _p(col), _p(val))
    return CsrHost(n, rp, col, val)


def matrix_a(N: int, bug_compat: bool = False) -> CsrHost:
    """Matrix_A<double>(N,N,N) + mult_diagonal (+ the as-run change_order) as CSR."""
    n, d, ix = matrix_a_ell(N, bug_compat)
    return ell_to_csr(n, 4, d, ix)


def rand_B(n: int, b: int, seed: int = 1, skip: int = 1, row_major: bool = True) -> np.ndarray:
    """random_matrix_B from the glibc rand() stream (after the lc draw)."""
    out = np.empty(n * b, np.float64)
    if host_lib().lzh_rand_B(n, b, seed, skip, int(row_major), _p(out)):
        raise LanczosError("lzh_rand_B failed")
    return out.reshape(n, b) if row_major else out.reshape(b, n).T


def rand_lc(seed: int = 1) -> int:
    return int(host_lib().lzh_rand_lc(seed))


def uniform_B(n: int, b: int, seed: int = 20261015, dtype=np.float64, r0: int = 0) -> np.ndarray:
    """Start block, uniform [1, 2) per row from a counter-based stream: rows
    [r0, r0 + n) of the global block (a rank's slab)."""
    out = np.empty((n, b), dtype)
    L = host_lib()
    if dtype == np.float64:
        L.lzh_uniform_B_rows(r0, n, b, seed, _p(out), None)
    else:
        L.lzh_uniform_B_rows(r0, n, b, seed, None, _p(out))
    return out


def sym_eig(A: np.ndarray, vectors: bool = False):
    A = np.ascontiguousarray(A, np.float64)
    k = A.shape[0]
    ev = np.empty(k)
    V = np.empty((k, k)) if vectors else None
    host_lib().lzh_sym_eig(k, _p(A), _p(ev), _p(V) if vectors else None)
    return (ev, V) if vectors else ev


def Assemble_T(m: int, b: int, alpha: np.ndarray, beta: np.ndarray) -> np.ndarray:
    T = np.empty((m * b, m * b))
    host_lib().lzh_assemble_T(m, b, _p(np.ascontiguousarray(alpha, np.float64)),
                              _p(np.ascontiguousarray(beta, np.float64)), _p(T))
    return T


def ritz_values(m: int, b: int, alpha: np.ndarray, beta: np.ndarray) -> np.ndarray:
    r = np.empty(m * b)
    host_lib().lzh_ritz_values(m, b, _p(np.ascontiguousarray(alpha, np.float64)),
                               _p(np.ascontiguousarray(beta, np.float64)), _p(r))
    return r


def ritz_pairs(m: int, b: int, alpha: np.ndarray, beta: np.ndarray, nev: int, which: str = "largest"):
    """Ritz pairs of Assemble_T(m, alpha, beta) (lzh_ritz_pairs): (theta[nev], S (m*b, nev),
    resid[nev]).  which = "smallest" (theta ascending) or "largest" (theta descending);
    beta holds m + 1 blocks with the true beta_m last (block_lanczos_reorth), and
    resid[i] = ||beta_m S[-b:, i]||."""
    if which not in ("smallest", "largest"):
        raise ValueError("which must be 'smallest' or 'largest'")
    beta = np.ascontiguousarray(beta, np.float64)
    if beta.size != (m + 1) * b * b:
        raise ValueError("beta must hold m + 1 blocks of b x b")
    theta, S, resid = np.empty(nev), np.empty((m * b, nev)), np.empty(nev)
    rc = host_lib().lzh_ritz_pairs(m, b, _p(np.ascontiguousarray(alpha, np.float64)), _p(beta), nev,
                                   0 if which == "smallest" else 1, _p(theta), _p(S), _p(resid))
    if rc:
        raise LanczosError("lzh_ritz_pairs failed (1 <= nev <= m*b)")
    return theta, S, resid


def _which(which: str, magnitude: bool = False) -> int:
    """lzh_*'s `which` of "smallest" / "largest"; magnitude: "magnitude" is accepted too (-1: the
    _mag functions, which take no `which`)."""
    if magnitude and which == "magnitude":
        return -1
    if which not in ("smallest", "largest"):
        raise ValueError("which must be 'smallest' or 'largest'" + (" or 'magnitude'" if magnitude else ""))
    return 0 if which == "smallest" else 1


def ritz_pairs_dense(m: int, b: int, T: np.ndarray, beta_m: np.ndarray, nev: int, which: str = "largest"):
    """ritz_pairs for a dense symmetric projected matrix T ((m*b, m*b), what a restarted
    solve has) and the b x b true beta_m of the final residual (lzh_ritz_pairs_dense):
    (theta[nev], S (m*b, nev), resid[nev]).  which = "magnitude" (lzh_ritz_pairs_dense_mag):
    |theta| descending, ties by theta ascending -- the wanted end of a shift-and-invert
    operator."""
    w = _which(which, magnitude=True)
    T = np.ascontiguousarray(T, np.float64)
    beta_m = np.ascontiguousarray(beta_m, np.float64)
    if T.shape != (m * b, m * b) or beta_m.size != b * b:
        raise ValueError("T must be (m*b, m*b) and beta_m (b, b)")
    theta, S, resid = np.empty(nev), np.empty((m * b, nev)), np.empty(nev)
    if w < 0:
        if host_lib().lzh_ritz_pairs_dense_mag(m, b, _p(T), _p(beta_m), nev, _p(theta), _p(S), _p(resid)):
            raise LanczosError("lzh_ritz_pairs_dense_mag failed (1 <= nev <= m*b)")
    elif host_lib().lzh_ritz_pairs_dense(m, b, _p(T), _p(beta_m), nev, w, _p(theta), _p(S), _p(resid)):
        raise LanczosError("lzh_ritz_pairs_dense failed (1 <= nev <= m*b)")
    return theta, S, resid


def restart_coeffs(m: int, b: int, r: int, T: np.ndarray, beta_m: np.ndarray, which: str = "largest"):
    """The host side of a thick restart that keeps the first r*b Ritz pairs of T
    (lzh_restart_coeffs): (theta_k[r*b], Z (r, m, b, b) in the layout of panel_compress,
    sigma (r, b, b) for block_lanczos_reorth_resume, T_next (m*b, m*b) with diag(theta_k)
    and the mirrored arrow block; restart_fill adds the resumed cycle's alpha / beta).
    which = "magnitude" (lzh_restart_coeffs_mag): the r*b pairs largest in |theta|."""
    w = _which(which, magnitude=True)
    T = np.ascontiguousarray(T, np.float64)
    beta_m = np.ascontiguousarray(beta_m, np.float64)
    if T.shape != (m * b, m * b) or beta_m.size != b * b:
        raise ValueError("T must be (m*b, m*b) and beta_m (b, b)")
    if not 1 <= r < m:
        raise LanczosError("lzh_restart_coeffs: 1 <= r < m")
    theta_k, Z, sigma, Tn = np.empty(r * b), np.empty((r, m, b, b)), np.empty((r, b, b)), np.empty((m * b, m * b))
    if w < 0:
        if host_lib().lzh_restart_coeffs_mag(m, b, r, _p(T), _p(beta_m), _p(theta_k), _p(Z), _p(sigma), _p(Tn)):
            raise LanczosError("lzh_restart_coeffs_mag failed")
    elif host_lib().lzh_restart_coeffs(m, b, r, _p(T), _p(beta_m), w, _p(theta_k), _p(Z), _p(sigma), _p(Tn)):
        raise LanczosError("lzh_restart_coeffs failed")
    return theta_k, Z, sigma, Tn


def restart_fill(r: int, m: int, b: int, alpha: np.ndarray, beta: np.ndarray, T_next: np.ndarray) -> np.ndarray:
    """T_next (from restart_coeffs, modified in place and returned) += the block-tridiagonal
    tail alpha_r, beta_{r+1}, alpha_{r+1}, ... of a resumed cycle (lzh_restart_fill)."""
    alpha = np.ascontiguousarray(alpha, np.float64)
    beta = np.ascontiguousarray(beta, np.float64)
    if T_next.dtype != np.float64 or not T_next.flags.c_contiguous or T_next.shape != (m * b, m * b) \
            or alpha.size < m * b * b or beta.size < m * b * b:
        raise ValueError("T_next must be a contiguous fp64 (m*b, m*b) array; alpha, beta hold m blocks")
    if host_lib().lzh_restart_fill(r, m, b, _p(alpha), _p(beta), _p(T_next)):
        raise LanczosError("lzh_restart_fill failed (1 <= r < m)")
    return T_next


def block_solution(m: int, b: int, T_end: float, alpha, beta, q) -> np.ndarray:
    s = np.empty(b)
    host_lib().lzh_block_solution(m, b, T_end, _p(np.ascontiguousarray(alpha, np.float64)),
                                  _p(np.ascontiguousarray(beta, np.float64)),
                                  _p(np.ascontiguousarray(q, np.float64)), _p(s))
    return s


def partition_rows(A: CsrHost, parts: int) -> np.ndarray:
    bounds = np.empty(parts + 1, np.int64)
    host_lib().lzh_partition_rows(A.n, _p(A.row_ptr), parts, _p(bounds))
    return bounds


def remap_cols_padded(col: np.ndarray, bounds: np.ndarray, n_pad: int) -> np.ndarray:
    col = np.ascontiguousarray(col, np.int32)
    out = np.empty_like(col)
    rc = host_lib().lzh_remap_cols_padded(col.size, _p(col), bounds.size - 1,
                                          _p(np.ascontiguousarray(bounds, np.int64)), n_pad, _p(out))
    if rc:
        raise LanczosError("lzh_remap_cols_padded failed")
    return out


def halo_plan(col: np.ndarray, bounds: np.ndarray, rank: int):
    """lzh_halo_plan: (compact columns, recv_counts[parts], halo_rows[n_halo]) for part
    `rank` of the row partition `bounds` (columns global on input)."""
    col = np.ascontiguousarray(col, np.int32)
    bounds = np.ascontiguousarray(bounds, np.int64)
    parts = bounds.size - 1
    out = np.empty_like(col)
    counts = np.zeros(parts, np.int64)
    rows = np.empty(max(col.size, 1), np.int32)
    nh = host_lib().lzh_halo_plan(col.size, _p(col), parts, _p(bounds), rank, _p(out), _p(counts), _p(rows))
    if nh < 0:
        raise LanczosError(f"lzh_halo_plan failed ({nh})")
    return out, counts, rows[:nh].copy()


def csr_write(path: str, A: CsrHost) -> None:
    dt = 0 if A.val.dtype == np.float64 else 1
    if host_lib().lzh_csr_write(path.encode(), A.n, A.n, A.nnz, _p(A.row_ptr), _p(A.col), _p(A.val), dt):
        raise LanczosError("lzh_csr_write failed")


def csr_read(path: str) -> CsrHost:
    L = host_lib()
    n, nc, nnz, dt = _c_i64(), _c_i64(), _c_i64(), _c_int()
    if L.lzh_csr_read_header(path.encode(), ctypes.byref(n), ctypes.byref(nc), ctypes.byref(nnz), ctypes.byref(dt)):
        raise LanczosError("bad CSR file")
    rp = np.empty(n.value + 1, np.int64)
    col = np.empty(nnz.value, np.int32)
    val = np.empty(nnz.value, np.float64 if dt.value == 0 else np.float32)
    if L.lzh_csr_read(path.encode(), _p(rp), _p(col), _p(val)):
        raise LanczosError("CSR read failed")
    return CsrHost(n.value, rp, col, val)


# ============================================================= GPU (torch)
def _torch():
    import torch  # plumbing: device memory + streams
    return torch


def _ld(t) -> int:
    """Leading dimension of a 2-D tensor (stride of a size-1 dim is arbitrary)."""
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise LanczosError("inner dimension must be contiguous")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dt(t) -> int:
    torch = _torch()
    if t.dtype == torch.float64:
        return LZ_F64
    if t.dtype == torch.float32:
        return LZ_F32
    raise LanczosError(f"unsupported dtype {t.dtype}")


@dataclass
class CsrDevice:
    """CSR operator resident in HBM (torch tensors on cuda)."""
    n: int
    n_cols: int
    row_ptr: "object"
    col: "object"
    val: "object"

    @property
    def nnz(self) -> int:
        return int(self.col.numel())

    @property
    def dtype(self) -> int:
        return _dt(self.val)

    @staticmethod
    def from_host(A: CsrHost, device="cuda", n_cols: Optional[int] = None) -> "CsrDevice":
        torch = _torch()
        return CsrDevice(A.n, A.n if n_cols is None else n_cols,
                         torch.from_numpy(A.row_ptr).to(device),
                         torch.from_numpy(A.col).to(device),
                         torch.from_numpy(A.val).to(device))

    def transpose(self, handle: "Handle") -> "CsrDevice":
        """The CSR of the transpose, built on the device (lz_csr_transpose): n and n_cols
        swapped, row c holding this operator's entries of column c in the order of their
        positions here.  Bitwise reproducible."""
        torch = _torch()
        dev = self.val.device
        t_rp = torch.empty(self.n_cols + 1, dtype=torch.int64, device=dev)
        t_col = torch.empty(self.nnz, dtype=torch.int32, device=dev)
        t_val = torch.empty(self.nnz, dtype=self.val.dtype, device=dev)
        _check(handle.L.lz_csr_transpose(handle.ptr, self.n, self.n_cols, self.nnz, _ptr(self.row_ptr), _ptr(self.col),
                                         _ptr(self.val), self.dtype, _ptr(t_rp), _ptr(t_col), _ptr(t_val)),
               "lz_csr_transpose")
        return CsrDevice(self.n_cols, self.n, t_rp, t_col, t_val)


class _ReorthOp(NamedTuple):
    """What Handle._reorth_op makes of A / filt / work / normal: fn(handle, *head, b, ..., passes, *tail)."""
    name: str                    # the ABI function
    head: tuple                  # n [, P.n], nnz, the CSR pointers [and the transpose's], dtype
    tail: tuple                  # nothing | &filt, work | work | degree, lo, hi, gamma, work | &inv, work, &info
    filt: object                 # the ChebFilter, gamma array or Inverse tail points to: alive as long as this description


def _f64(t) -> np.ndarray:
    """A device tensor copied back to the host, as fp64."""
    return t.cpu().numpy().astype(np.float64)


def _panel_stride(rows: int, b: int, like) -> int:
    """The stride of a panel of (rows, b) blocks of like's dtype: every block on 16 bytes."""
    per16 = 16 // like.element_size()
    return -(-rows * b // per16) * per16


def _pack_chunks(S: np.ndarray, m: int, b: int) -> np.ndarray:
    """Host coefficients S (m*b, nev) in panel_compress's layout: (ceil(nev / b), m, b, b),
    chunk c holding columns [c*b, (c+1)*b) of S, the last zero-padded."""
    nev = S.shape[1]
    nch = -(-nev // b)
    Sp = np.zeros((nch, m, b, b))
    for c in range(nch):
        w = min(b, nev - c * b)
        Sp[c, :, :, :w] = S[:, c * b:c * b + w].reshape(m, b, w)
    return Sp


def rank_ratios(beta: np.ndarray, j0: int, T: np.ndarray) -> np.ndarray:
    """The rank ratio of the fresh blocks beta[j0:] ((m + 1, b, b), host fp64) of a cycle:
    sigma_min(beta_j) / max|theta(T)|, T the cycle's projected matrix; for the start block's
    beta_0, which T does not hold, sigma_min / sigma_max.  NaN where beta_j (or, past beta_0,
    T) is not finite or the denominator is zero.  A block W = Q_j beta_j of full rank whose
    columns are as long as the operator is wide has a ratio of order 1 / b; a singular W^T W
    gives one near sqrt(eps) or below (its computed zero eigenvalue over the largest)."""
    out = np.full(len(beta) - j0, np.nan)
    scale = None
    for i, bj in enumerate(beta[j0:]):
        if not np.isfinite(bj).all():
            continue
        sv = np.linalg.svd(bj, compute_uv=False)
        if j0 + i == 0:
            den = sv[0]
        else:
            if scale is None:
                scale = float(np.abs(np.linalg.eigvalsh(0.5 * (T + T.T))).max()) if np.isfinite(T).all() else np.nan
            den = scale
        if den > 0:  # (False for NaN)
            out[i] = sv[-1] / den
    return out


def _restart_sizes(who: str, count: str, nev: int, b: int, m: Optional[int], keep: Optional[int],
                   n: Optional[int] = None):
    """(m, keep) of a thick-restart solve for nev pairs, with the defaults and limits of
    eigsh's docstring; who and count name the caller and its nev in the errors.  n: the
    Lanczos dimension; a panel of m * b orthonormal columns needs m * b <= n."""
    want = -(-(nev + b) // b)  # the smallest keep with keep * b >= nev + b
    if m is None:
        m = min(PANEL_MAX_BLOCKS, max(4, 2 * want))
    r = min(want, PANEL_MAX_KEEP, m - 1) if keep is None else keep
    if nev < 1 or r * b < nev:
        raise LanczosError(f"{who}: keep * b = {r * b} < {count} = {nev}")
    if r >= m:
        raise LanczosError(f"{who}: keep = {r} >= m = {m}")
    if r > PANEL_MAX_KEEP or m > PANEL_MAX_BLOCKS or r < 1:
        raise LanczosError(f"{who}: 1 <= keep <= {PANEL_MAX_KEEP} and m <= {PANEL_MAX_BLOCKS}")
    if n is not None and m * b > n:
        raise LanczosError(f"{who}: m * b = {m * b} > n = {n}: the panel cannot hold more orthonormal columns "
                           f"than the operator has rows")
    return m, r


class _Restart:
    """The thick-restart loop that eigsh, its filtered form and svds share, as steps: it owns
    the panel V (m blocks of (n, b), vstride apart), W, q / al / be with their host copies
    alpha / beta, the projected matrix T, the operator keywords op (filt + work, series + work,
    inverse + work, or normal: one operator for every cycle of a solve; only the keywords the
    caller set are passed on) and the counters.  which: "smallest", "largest" or, on an
    inverse, "magnitude".

        first(B)         block_lanczos_reorth from B, copy back, Assemble_T, check_rank
        ritz(which)      all m*b Ritz pairs of T: theta, S, resid, max|theta|
        compress(which)  restart_coeffs, then panel_compress onto the keep*b kept pairs
        resume()         row lc of the kept blocks into q, block_lanczos_reorth_resume,
                         copy back, restart_fill, check_rank
        pack(S, nev)     panel_compress onto the Ritz vectors of S[:, :nev]; returns their blocks

    One copy-back each of q, al and be per cycle; the callers keep the stop test.  check_rank
    refuses a cycle with a rank-deficient fresh block (LanczosError); ran, when set, is called
    after the cycle's device call and before that test."""

    def __init__(self, h: "Handle", A, n: int, b: int, m: int, r: int, lc: int, passes: int, like, **op):
        torch = _torch()
        self.h, self.A, self.n, self.b, self.m, self.r = h, A, n, b, m, r
        self.lc, self.passes, self.op = lc, passes, op
        self.kw = kw = dict(dtype=like.dtype, device=like.device)
        self.npdt = np.float64 if like.dtype == torch.float64 else np.float32
        self.delta = (RANK_DELTA_START_F64, RANK_DELTA_STEP_F64) if like.dtype == torch.float64 \
            else (RANK_DELTA_START_F32, RANK_DELTA_STEP_F32)  # (beta_0, every later block)
        self.ran = None  # called after every cycle's device call, before its rank test
        self.vstride = _panel_stride(n, b, like)
        self.V = torch.zeros(m * self.vstride, **kw)
        self.W = torch.empty(n, b, **kw)
        self.q = torch.zeros(m * b, **kw)
        self.al, self.be = torch.zeros(m, b, b, **kw), torch.zeros(m + 1, b, b, **kw)
        self.steps = self.cycles = 0  # Lanczos steps of every solve on these buffers; cycles of the last first()

    def start_block(self, B):
        """B, or the default start block uniform_B(n, b) on the device."""
        if B is not None:
            return B
        return _torch().from_numpy(uniform_B(self.n, self.b, dtype=self.npdt)).to(self.kw["device"])

    def _dev(self, a: np.ndarray):
        return _torch().from_numpy(a).to(**self.kw)

    def first(self, B):
        self.h.block_lanczos_reorth(self.A, B, self.m, self.lc, self.q, self.al, self.be, self.V, self.vstride, self.W,
                                    passes=self.passes, **self.op)
        self.steps += self.m
        self.cycles = 1
        self.alpha, self.beta = _f64(self.al), _f64(self.be)
        self.T = Assemble_T(self.m, self.b, self.alpha, self.beta[:self.m])
        if self.ran:
            self.ran()
        self.check_rank(0)

    def check_rank(self, j0: int):
        """Refuse a cycle whose fresh blocks beta[j0:] are rank deficient (rank_ratios below
        delta, or not finite): beta^-1 = 1 / sqrt|lambda| then left the panel unnormalised and
        not orthogonal, and neither T nor the residual estimate beta_m S[-b:] means anything.
        Host work on the copies first() and resume() already made."""
        for i, x in enumerate(rank_ratios(self.beta, j0, self.T)):
            j = j0 + i
            delta = self.delta[min(j, 1)]
            if not x >= delta:  # (NaN fails)
                where = "the start block" if j == 0 else f"the block of cycle {self.cycles}, step {j}"
                raise LanczosError(f"{where} is rank deficient (rank ratio {x:.1e} < {delta:.1e}): its columns "
                                   f"are dependent to working precision, or the Krylov space is exhausted")

    def ritz(self, which: str):
        theta, S, resid = ritz_pairs_dense(self.m, self.b, self.T, self.beta[self.m], self.m * self.b, which)
        return theta, S, resid, float(np.abs(theta).max())

    def compress(self, which: str):
        _, self.Z, self.sigma, self.T = restart_coeffs(self.m, self.b, self.r, self.T, self.beta[self.m], which)
        self.h.panel_compress(self.V, self.vstride, self.m, self.r, self._dev(self.Z), n=self.n)

    def resume(self):
        m, b, r = self.m, self.b, self.r
        # row lc of Y = P Z_k
        Zk = self.Z.transpose(1, 2, 0, 3).reshape(m * b, r * b)
        self.q[:r * b] = self._dev(_f64(self.q) @ Zk)
        self.h.block_lanczos_reorth_resume(self.A, r, m, self.lc, self._dev(self.sigma), self.q, self.al, self.be,
                                           self.V, self.vstride, self.W, passes=self.passes, **self.op)
        self.alpha, self.beta = _f64(self.al), _f64(self.be)
        restart_fill(r, m, b, self.alpha, self.beta, self.T)
        self.steps += m - r
        self.cycles += 1
        if self.ran:
            self.ran()
        self.check_rank(r)

    def pack(self, S: np.ndarray, nev: int) -> int:
        Zx = _pack_chunks(S[:, :nev], self.m, self.b)
        self.h.panel_compress(self.V, self.vstride, self.m, len(Zx), self._dev(Zx), n=self.n)
        return len(Zx)


class Handle:
    """lz_handle on one device, bound to torch's current stream at each call."""

    def __init__(self, device: int = 0):
        L = hip_lib()
        if not L.lz_device_ok(device):
            raise LanczosError(f"no gfx950 device {device} visible to liblz_hip.so")
        h = _c_vp()
        _check(L.lz_init(device, ctypes.byref(h)), "lz_init")
        self._h = h
        self.device = device
        self.L = L

    def close(self):
        if self._h:
            self.L.lz_finalize(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        _check(self.L.lz_set_stream(self._h, _c_vp(s)), "lz_set_stream")

    @property
    def ptr(self):
        self._sync_stream()
        return self._h

    # --- operator API (reference names) -------------------------------
    def spmm(self, A: CsrDevice, X, Y, layout: int = LZ_ROW_MAJOR):
        """Y = A*X (kernels/spmv_spmm.hpp:262-333). X/Y (rows, b) row-major tensors, or
        column-major (b, rows) tensors viewed transposed when layout=LZ_COL_MAJOR."""
        b = X.shape[1] if layout == LZ_ROW_MAJOR else X.shape[0]
        ldx, ldy = _ld(X), _ld(Y)
        _check(self.L.lz_csr_spmm(self.ptr, A.n, A.n_cols, A.nnz, _ptr(A.row_ptr), _ptr(A.col),
                                  _ptr(A.val), A.dtype, b, _ptr(X), ldx, layout, _ptr(Y), ldy), "lz_csr_spmm")
        return Y

    def _blocks(self, what: str, A: CsrDevice, *ts):
        """n x b contiguous blocks of A's dtype for the three-term step and the filter."""
        n, b = ts[0].shape
        if A.n != A.n_cols or n != A.n:
            raise LanczosError(f"{what}: a square operator with as many rows as the blocks")
        for t in ts:
            if t is not None and (tuple(t.shape) != (n, b) or not t.is_contiguous() or t.dtype != A.val.dtype):
                raise LanczosError(f"{what}: every block (n, b) contiguous (ld = b), of A's dtype")
        return n, b

    def spmm_axpby(self, A: CsrDevice, a: float, X, c: float, d: float, Z, Y):
        """Y = a (A X) + c X + d Z (lz_csr_spmm_axpby): A square, X / Z / Y (n, b) contiguous and
        pairwise distinct; d == 0 never reads Z, which may be None."""
        n, b = self._blocks("spmm_axpby", A, X, Y, Z)
        _check(self.L.lz_csr_spmm_axpby(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                        a, _ptr(X), c, d, _ptr(Z), _ptr(Y)), "lz_csr_spmm_axpby")
        return Y

    def spmm_axpby4(self, A: CsrDevice, a: float, X, c: float, d: float, Z, e: float, U, Y):
        """Y = a (A X) + c X + d Z + e U (lz_csr_spmm_axpby4): spmm_axpby with a fourth term, the
        step of Clenshaw's recurrence.  Y is distinct from X, Z and U; U may be X or Z.  d == 0
        never reads Z and e == 0 never reads U; either may then be None."""
        n, b = self._blocks("spmm_axpby4", A, X, Y, Z, U)
        _check(self.L.lz_csr_spmm_axpby4(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                         a, _ptr(X), c, d, _ptr(Z), e, _ptr(U), _ptr(Y)), "lz_csr_spmm_axpby4")
        return Y

    def spmm_rowscale(self, A: CsrDevice, s, a: float, g: float, X, e: float, U, c: float, d: float, Z, Y,
                      dots=None, want_dots: bool = True):
        """Y[i] = s_i (a (A X)[i] + g X[i] + e U[i]) + c X[i] + d Z[i] (lz_csr_spmm_rowscale), the step
        of the Jacobi-scaled Chebyshev preconditioner.  s: n elements of A's dtype; X, U, Z, Y (n, b)
        contiguous, Y distinct from the others; U is required, d == 0 never reads Z, which may then
        be None.  Returns (Y, dots): the column dots of the stored Y with itself and with U as
        col_dots(Y, U) returns them; want_dots=False: no dots are formed and dots is None."""
        torch = _torch()
        if U is None:
            raise LanczosError("spmm_rowscale: U is required (LZ_E_ARG)")
        n, b = self._blocks("spmm_rowscale", A, X, Y, Z, U)
        if not torch.is_tensor(s) or s.dim() != 1 or s.numel() != n or s.dtype != A.val.dtype or not s.is_contiguous() \
                or s.device != X.device:
            raise LanczosError("spmm_rowscale: s is a contiguous 1-D device tensor of n elements of A's dtype (LZ_E_ARG)")
        if want_dots:
            dots = self._dots("spmm_rowscale", dots, 1, b, Y)
        _check(self.L.lz_csr_spmm_rowscale(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                           _ptr(s), a, g, _ptr(X), e, _ptr(U), c, d, _ptr(Z), _ptr(Y),
                                           _ptr(dots) if want_dots else None), "lz_csr_spmm_rowscale")
        return Y, (dots.view(2, b) if want_dots else None)

    def spmm_axpby4_dots(self, A: CsrDevice, a: float, X, c: float, d: float, Z, e: float, U, Y, dots=None):
        """spmm_axpby4 with U required (e != 0), and the column dots of the stored Y with itself and
        with U as col_dots(Y, U) returns them (lz_csr_spmm_axpby4_dots); returns (Y, dots)."""
        n, b = self._blocks("spmm_axpby4_dots", A, X, Y, Z, U)
        dots = self._dots("spmm_axpby4_dots", dots, 1, b, Y)
        _check(self.L.lz_csr_spmm_axpby4_dots(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                              a, _ptr(X), c, d, _ptr(Z), e, _ptr(U), _ptr(Y), _ptr(dots)),
               "lz_csr_spmm_axpby4_dots")
        return Y, dots.view(2, b)

    def _dots(self, what: str, dots, rows: int, b: int, like):
        """The (rows, 2, b) fp64 device tensor the dots land in (allocated when None)."""
        torch = _torch()
        if dots is None:
            return torch.empty(rows, 2, b, dtype=torch.float64, device=like.device)
        if dots.dtype != torch.float64 or not dots.is_contiguous() or dots.numel() != rows * 2 * b:
            raise LanczosError(f"{what}: dots is a contiguous fp64 tensor of {rows} x 2 x b elements")
        return dots

    def col_dots(self, Y, X, dots=None):
        """dots[0] = the column sums of Y * Y, dots[1] = those of Y * X (lz_col_dots): Y, X (n, b)
        contiguous, of one dtype, b <= 64; fp64 sums in a fixed order, on the device.  Y may be X."""
        n, b = Y.shape
        if tuple(X.shape) != (n, b) or X.dtype != Y.dtype or not (X.is_contiguous() and Y.is_contiguous()):
            raise LanczosError("col_dots: Y and X (n, b) contiguous (ld = b), of one dtype")
        dots = self._dots("col_dots", dots, 1, b, Y)
        _check(self.L.lz_col_dots(self.ptr, n, b, _dt(Y), _ptr(Y), _ptr(X), _ptr(dots)), "lz_col_dots")
        return dots.view(2, b)

    def spmm_axpby_dots(self, A: CsrDevice, a: float, X, c: float, d: float, Z, Y, dots=None):
        """spmm_axpby, and the column dots of the stored Y with itself and with X as col_dots
        returns them (lz_csr_spmm_axpby_dots); returns (Y, dots)."""
        n, b = self._blocks("spmm_axpby_dots", A, X, Y, Z)
        dots = self._dots("spmm_axpby_dots", dots, 1, b, Y)
        _check(self.L.lz_csr_spmm_axpby_dots(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                             a, _ptr(X), c, d, _ptr(Z), _ptr(Y), _ptr(dots)), "lz_csr_spmm_axpby_dots")
        return Y, dots.view(2, b)

    def spmm_resid(self, A: CsrDevice, X, theta, R, dots=None):
        """R = A X - X diag(theta) and the column dots of the stored R with itself and with X
        (lz_csr_spmm_resid): the residual block of b Ritz pairs in one pass.  theta: b fp64
        elements on the device, each rounded to A's dtype once; X (read only) and R (n, b)
        contiguous and distinct.  With every theta equal it is spmm_axpby_dots(A, 1, X, -theta, 0,
        None, R) bit for bit.  Returns (R, dots); dots[0] = the squared residual norms."""
        torch = _torch()
        n, b = self._blocks("spmm_resid", A, X, R)
        if not torch.is_tensor(theta) or theta.dtype != torch.float64 or not theta.is_contiguous() \
                or theta.numel() != b or theta.device != X.device:
            raise LanczosError("spmm_resid: theta is a contiguous fp64 device tensor of b elements")
        dots = self._dots("spmm_resid", dots, 1, b, R)
        _check(self.L.lz_csr_spmm_resid(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                        _ptr(theta), _ptr(X), _ptr(R), _ptr(dots)), "lz_csr_spmm_resid")
        return R, dots.view(2, b)

    def cheb_moments(self, A: CsrDevice, X0, K: int, lo: float, hi: float, work=None, dots=None):
        """The raw dots of K Chebyshev steps from X0 on (A - c0) / e, [lo, hi] = [c0 - e, c0 + e]
        enclosing A's spectrum (lz_cheb_moments): a (K+1, 2, b) fp64 device tensor, row k =
        (<t_k,t_k>, <t_k,t_{k-1}>), row 0 = (<t_0,t_0>, 0); kpm_moments turns it into 2K+1
        moments.  work: flat, 3*n*b elements (allocated when None); X0 is only read."""
        torch = _torch()
        n, b = self._blocks("cheb_moments", A, X0)
        if work is None:
            work = torch.empty(3 * n * b, dtype=X0.dtype, device=X0.device)
        if work.dim() != 1 or not work.is_contiguous() or work.numel() < 3 * n * b or work.dtype != X0.dtype:
            raise LanczosError("cheb_moments: work is a flat contiguous tensor of 3*n*b elements of X0's dtype")
        dots = self._dots("cheb_moments", dots, max(int(K), 0) + 1, b, X0)
        _check(self.L.lz_cheb_moments(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                      lo, hi, K, _ptr(X0), _ptr(work), _ptr(dots)), "lz_cheb_moments")
        return dots.view(-1, 2, b)

    @staticmethod
    def _cg_update_args(what: str, names: str, blocks, coef, dots_name: str, dots, k: int, dinv=None):
        """cg_update's and pcg_update's checks: the blocks, coef, dinv when there is one, and the dots
        (k b fp64, allocated when None), which it returns."""
        torch = _torch()
        like = blocks[0]
        n, b = like.shape
        for t in blocks:
            if tuple(t.shape) != (n, b) or t.dtype != like.dtype or not t.is_contiguous():
                raise LanczosError(f"{what}: {names} (n, b) contiguous (ld = b), of one dtype")
        if coef.dtype != torch.float64 or not coef.is_contiguous() or coef.numel() != 2 * b:
            raise LanczosError(f"{what}: coef is a contiguous fp64 tensor of 2 b elements")
        if dinv is not None and (dinv.dim() != 1 or dinv.numel() != n or dinv.dtype != like.dtype
                                 or not dinv.is_contiguous()):
            raise LanczosError(f"{what}: dinv is a contiguous 1-D tensor of n elements of the blocks' dtype")
        if dots is None:
            dots = torch.empty(k * b, dtype=torch.float64, device=like.device)
        if dots.dtype != torch.float64 or not dots.is_contiguous() or dots.numel() != k * b:
            size = "2 b" if k == 2 else "b"
            raise LanczosError(f"{what}: {dots_name} is a contiguous fp64 tensor of {size} elements")
        return dots

    def cg_update(self, coef, R, W, P, S, X, rr=None):
        """The row-local half of one conjugate-gradient step with per-column device coefficients
        (lz_cg_update): P = R + beta P, S = W + beta S, X += alpha P, R -= alpha S, each element
        finished as one fma in that order, and rr[c] = the column sums of the new R * R in fp64.
        coef: 2 b fp64 on the device, [alpha(b) | beta(b)], read only, rounded once to the blocks'
        dtype; R, W (read only), P, S, X: (n, b) contiguous, of one dtype, pairwise distinct; a zero
        coefficient skips its product.  Returns rr (b fp64 on the device; allocated when None)."""
        n, b = R.shape
        rr = self._cg_update_args("cg_update", "R, W, P, S, X", (R, W, P, S, X), coef, "rr", rr, 1)
        _check(self.L.lz_cg_update(self.ptr, n, b, _dt(R), _ptr(coef), _ptr(R), _ptr(W), _ptr(P), _ptr(S), _ptr(X),
                                   _ptr(rr)), "lz_cg_update")
        return rr

    def pcg_update(self, coef, dinv, R, W, P, S, X, Z, dots=None):
        """cg_update with a diagonal preconditioner (lz_pcg_update): with dv = dinv[row], P = dv R +
        beta P, S = W + beta S, X += alpha P, R -= alpha S, Z = dv R (the new R), each finished in that
        order under cg_update's zero-coefficient rules; Z is written, never read.  dinv: n elements of
        the blocks' dtype, read only; R, W (read only), P, S, X, Z: (n, b) contiguous, of one dtype, all
        seven pairwise distinct.  Returns dots (2 b fp64 on the device, [R.Z (b) | R.R (b)] of the
        stored values; allocated when None)."""
        n, b = R.shape
        dots = self._cg_update_args("pcg_update", "R, W, P, S, X, Z", (R, W, P, S, X, Z), coef, "dots", dots, 2, dinv)
        _check(self.L.lz_pcg_update(self.ptr, n, b, _dt(R), _ptr(coef), _ptr(dinv), _ptr(R), _ptr(W), _ptr(P),
                                    _ptr(S), _ptr(X), _ptr(Z), _ptr(dots)), "lz_pcg_update")
        return dots

    def cgz_update(self, coef, R, W, P, S, X, Z, rr=None):
        """cg_update with z0 read from the block Z (lz_cgz_update): P = Z + beta P, S = W + beta S, X +=
        alpha P, R -= alpha S under cg_update's zero-coefficient rules, and rr[c] = the column sums of
        the new R * R.  Z and W are read only and nothing is written to Z; R, W, P, S, X, Z: (n, b)
        contiguous, of one dtype, all six pairwise distinct.  Returns rr (b fp64 on the device)."""
        n, b = R.shape
        rr = self._cg_update_args("cgz_update", "R, W, P, S, X, Z", (R, W, P, S, X, Z), coef, "rr", rr, 1)
        _check(self.L.lz_cgz_update(self.ptr, n, b, _dt(R), _ptr(coef), _ptr(R), _ptr(W), _ptr(P), _ptr(S), _ptr(X),
                                    _ptr(Z), _ptr(rr)), "lz_cgz_update")
        return rr

    def cgzs_update(self, coef, dinv, R, W, P, S, X, Z, Rs, rr=None):
        """cgz_update that also writes Rs = dinv[:, None] * R of the stored R (lz_cgzs_update), the
        update pass of the Jacobi-scaled Chebyshev preconditioner: the same bits in R, P, S, X and rr;
        one rounded product per element of Rs, a frozen column's rewritten with the bits it held.
        dinv: n elements of the blocks' dtype, read only; R, W, P, S, X, Z, Rs: (n, b) contiguous, of
        one dtype, all seven pairwise distinct.  Returns rr (b fp64 on the device)."""
        n, b = R.shape
        rr = self._cg_update_args("cgzs_update", "R, W, P, S, X, Z, Rs", (R, W, P, S, X, Z, Rs), coef, "rr", rr, 1,
                                  dinv)
        _check(self.L.lz_cgzs_update(self.ptr, n, b, _dt(R), _ptr(coef), _ptr(dinv), _ptr(R), _ptr(W), _ptr(P),
                                     _ptr(S), _ptr(X), _ptr(Z), _ptr(Rs), _ptr(rr)), "lz_cgzs_update")
        return rr

    def cheb_precond_apply(self, A: CsrDevice, precond, R, Z, work=None, shift: float = 0.0, dots=None, dinv=None):
        """Z = q(A + shift I) R, q the Chebyshev polynomial preconditioner `precond` (a ChebPrecond
        with lo and hi given, or (degree, lo, hi)), in exactly degree SpMMs (lz_cheb_precond_apply).
        work: flat, 2*n*b elements (allocated when None); R is only read.  Returns (Z, dots): dots[0] =
        the column sums of Z * Z, dots[1] = those of Z * R, of the stored Z.
        dinv (n elements of A's dtype): the Jacobi-scaled form Z = q(D^-1 M) D^-1 R with D^-1 = dinv
        (lz_cheb_jacobi_apply), [lo, hi] enclosing D^-1/2 M D^-1/2; Rs = dinv[:, None] * R is formed
        here, one rounded product per element."""
        torch = _torch()
        n, b = self._blocks("cheb_precond_apply", A, R, Z)
        pc = _cheb_precond(precond)
        if work is None:
            work = torch.empty(2 * n * b, dtype=R.dtype, device=R.device)
        self._work("cheb_precond_apply", work, n, b, R)
        dots = self._dots("cheb_precond_apply", dots, 1, b, Z)
        if dinv is not None:
            if not torch.is_tensor(dinv) or dinv.dim() != 1 or dinv.numel() != n or dinv.dtype != R.dtype \
                    or not dinv.is_contiguous() or dinv.device != R.device:
                raise LanczosError("cheb_precond_apply: dinv is a contiguous 1-D device tensor of n elements of A's dtype")
            Rs = dinv[:, None] * R
            _check(self.L.lz_cheb_jacobi_apply(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype,
                                               b, float(shift), ctypes.addressof(pc), _ptr(dinv), _ptr(R), _ptr(Rs),
                                               _ptr(Z), _ptr(work), _ptr(dots)), "lz_cheb_jacobi_apply")
            return Z, dots.view(2, b)
        _check(self.L.lz_cheb_precond_apply(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                            float(shift), ctypes.addressof(pc), _ptr(R), _ptr(Z), _ptr(work),
                                            _ptr(dots)), "lz_cheb_precond_apply")
        return Z, dots.view(2, b)

    def jacobi(self, A: CsrDevice, shift: float = 0.0):
        """The Jacobi preconditioner of A + shift I (lz_csr_jacobi): dinv[i] = 1 / (a_ii + shift) in
        A's dtype, a_ii the sum of row i's stored diagonal entries (none: 0), shift rounded once to
        that dtype.  Raises LanczosError, naming the count, when a row's diagonal is not positive and
        finite: such an operator is not positive definite."""
        torch = _torch()
        if A.n_cols != A.n:
            raise LanczosError("jacobi: A is square")
        dinv = torch.empty(A.n, dtype=A.val.dtype, device=A.val.device)
        bad = _c_i64(-1)
        _check(self.L.lz_csr_jacobi(self.ptr, A.n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype,
                                    float(shift), _ptr(dinv), ctypes.addressof(bad)), "lz_csr_jacobi")
        if bad.value:
            raise LanczosError(f"jacobi: {bad.value} rows of A + shift I have a diagonal that is not positive and finite")
        return dinv

    def _bcg_factors(self, what: str, b: int, *ms):
        torch = _torch()
        for m in ms:
            if m.dtype != torch.float64 or not m.is_contiguous() or m.numel() != b * b:
                raise LanczosError(f"{what}: the b x b factors are contiguous fp64 tensors on the device")

    def bcg_update(self, xi, E, S, W, Q, X, G=None):
        """The update pass of one block conjugate-gradient iteration (lz_bcg_update): X += S E, Q -= W xi
        and G = Q^T Q of the stored Q (b x b fp64 on the device; allocated when None).  xi, E: b x b
        fp64 on the device, read only, rounded once to the blocks' dtype; S, W (read only), Q, X: (n, b)
        contiguous, of one dtype, pairwise distinct, b <= BCG_MAX_B.  Returns G."""
        torch = _torch()
        n, b = S.shape
        for t in (S, W, Q, X):
            if tuple(t.shape) != (n, b) or t.dtype != S.dtype or not t.is_contiguous():
                raise LanczosError("bcg_update: S, W, Q, X (n, b) contiguous (ld = b), of one dtype")
        self._bcg_factors("bcg_update", b, xi, E)
        if G is None:
            G = torch.empty(b, b, dtype=torch.float64, device=S.device)
        self._bcg_factors("bcg_update", b, G)
        _check(self.L.lz_bcg_update(self.ptr, n, b, _dt(S), _ptr(xi), _ptr(E), _ptr(S), _ptr(W), _ptr(Q), _ptr(X),
                                    _ptr(G)), "lz_bcg_update")
        return G

    def bcg_direction(self, z, zinv, Q, S):
        """The direction pass of one block conjugate-gradient iteration (lz_bcg_direction): Q <- Q zinv,
        then S <- Q + S z with the new Q, in place.  z (symmetric), zinv: b x b fp64 on the device; Q, S:
        (n, b) contiguous, of one dtype, distinct."""
        n, b = Q.shape
        if tuple(S.shape) != (n, b) or S.dtype != Q.dtype or not S.is_contiguous() or not Q.is_contiguous():
            raise LanczosError("bcg_direction: Q, S (n, b) contiguous (ld = b), of one dtype")
        self._bcg_factors("bcg_direction", b, z, zinv)
        _check(self.L.lz_bcg_direction(self.ptr, n, b, _dt(Q), _ptr(z), _ptr(zinv), _ptr(Q), _ptr(S)),
               "lz_bcg_direction")

    def minres_update(self, coef, W, U, Uo, D1, D2, X, uu=None):
        """The row-local half of one MINRES pass with per-column device coefficients (lz_minres_update):
        u' = a_w W + a_u U + a_o Uo, d' = g_o Uo + g_1 D1 + g_2 D2, X += tau d', each element finished as
        a product and fmas in that order, u' stored into Uo and d' into D2, and uu[c] = the column sums
        of the stored u' * u' in fp64.  coef: 7 b fp64 on the device, [a_w | a_u | a_o | g_o | g_1 | g_2 |
        tau] of b entries each, read only, rounded once to the blocks' dtype; W, U, D1 (read only), Uo,
        D2, X: (n, b) contiguous, of one dtype, pairwise distinct; a zero coefficient skips its term
        whatever its operand holds.  Returns uu (b fp64 on the device; allocated when None)."""
        torch = _torch()
        n, b = W.shape
        for t in (W, U, Uo, D1, D2, X):
            if tuple(t.shape) != (n, b) or t.dtype != W.dtype or not t.is_contiguous():
                raise LanczosError("minres_update: W, U, Uo, D1, D2, X (n, b) contiguous (ld = b), of one dtype")
        if coef.dtype != torch.float64 or not coef.is_contiguous() or coef.numel() != MINRES_COEFS * b:
            raise LanczosError("minres_update: coef is a contiguous fp64 tensor of 7 b elements")
        if uu is None:
            uu = torch.empty(b, dtype=torch.float64, device=W.device)
        if uu.dtype != torch.float64 or not uu.is_contiguous() or uu.numel() != b:
            raise LanczosError("minres_update: uu is a contiguous fp64 tensor of b elements")
        _check(self.L.lz_minres_update(self.ptr, n, b, _dt(W), _ptr(coef), _ptr(W), _ptr(U), _ptr(Uo), _ptr(D1),
                                       _ptr(D2), _ptr(X), _ptr(uu)), "lz_minres_update")
        return uu

    def solve(self, A: CsrDevice, B, shift: float = 0.0, tol: Optional[float] = None, max_iter: Optional[int] = None,
              X0=None, check_every: Optional[int] = None, max_restarts: int = 3, work=None,
              method: str = "columns", precond=None):
        """Solves (A + shift I) X = B for a symmetric positive definite A + shift I by conjugate
        gradients, the b <= 64 columns of B in lock step, each by its own scalars (lz_cg_solve).

        The precision is A's: blocks and the SpMM run in A's dtype (shift is rounded to it once), the
        dots and the scalars in fp64.  tol: the relative residual |B_c - M X_c| / |B_c| a column must
        reach, default 1e-10 for an fp64 operator and 1e-4 for fp32; max_iter: most steps of one
        column, default min(10 n, 10000); X0: the start block, default zeros (it is copied, not
        overwritten).  Device memory: 6 blocks of n b elements (B, X and the four of work: flat,
        4 n b elements, allocated when None).  Without a preconditioner the iterations grow like
        the square root of the condition number.  Per iteration: one fused SpMM with dots, one
        scalar launch and one update pass; the host reads one live count per check_every iterations
        (default: the library's, CG_CHECK_EVERY).  A converged column is frozen and its X no longer
        changes by a bit; when all are frozen the true residual is measured and columns that fail
        it run again from it, at most max_restarts times.  A column whose B holds a NaN ends at
        once with status 2 (its denominator is not finite), its X untouched.

        method="block" (lz_bcg_solve, b <= BCG_MAX_B): block conjugate gradients, the columns
        sharing one Krylov space, so the rate follows lambda_max / lambda_b instead of lambda_max /
        lambda_1 -- fewer iterations on Laplacian-like operators, none fewer (and more work per
        iteration) on a well-conditioned one.  Same arguments; iters is the block's count for
        every column; status 2 is the block's diagnosis, given to every column that is not met.
        A start or restart whose residual block is rank deficient (a zero or duplicated column,
        b > n, an exhausted Krylov space) hands the rest to the column method (fallback = 1).

        precond (lz_pcg_solve; method="columns" only): a diagonal preconditioner D^-1, z = D^-1 r.
        None (the default): none, today's path and today's bits.  "jacobi": D = the diagonal of A +
        shift I (Handle.jacobi; it raises when a row's diagonal is not positive).  A 1-D tensor of n
        positive elements of A's dtype: that D^-1.  A column still stops on the true residual
        |B_c - M X_c| <= tol |B_c|, and status 2 also covers a D^-1 that is not positive.  Jacobi
        pays where the diagonal varies over orders of magnitude (a variable coefficient or mass, a
        reaction term, a power-law graph's degrees): 3 to 40 times fewer iterations there, each
        with one more block stream.  On a constant diagonal -- a plain Laplacian, a banded operator
        with a near-constant diagonal -- Jacobi gains nothing: the same iterations, each a little
        slower.  work is then 5 n b elements (PCG_WORK_BLOCKS), and the device holds 7 blocks and dinv.

        precond=ChebPrecond(degree=8, lo=None, hi=None), or "chebyshev" for ChebPrecond()
        (lz_pcg_cheb_solve; method="columns" only): the Chebyshev polynomial preconditioner z = q(M) r
        of that degree on [lo, hi], degree SpMMs per application.  hi=None: gershgorin(A)[1] + shift (one
        copy of the CSR arrays to the host), a guaranteed upper bound, with which q(M) is positive
        definite whatever lo is; lo=None: hi / (4 (degree + 1)^2) (cheb_precond_lo).  It pays where
        Jacobi cannot -- a constant diagonal, the grid Laplacians and banded operators: about degree +
        1 times fewer iterations for about the same SpMMs, each iteration one update pass, one scalar
        launch and one live-count read.  A caller who knows lambda_min passes it as lo; an hi below
        lambda_max makes q indefinite and ends columns with status 2.  work is then 7 n b elements
        (CHEB_PCG_WORK_BLOCKS); n_spmm = (degree + 1) iterations + starts + degree (starts with a live
        column).  The dict carries precond="chebyshev", precond_degree and precond_bounds=(lo, hi).

        precond=ChebPrecond(..., jacobi=True), or "jacobi-chebyshev" for ChebPrecond(jacobi=True)
        (lz_pcg_cheb_jacobi_solve; method="columns" only): the two combined, z = q(D^-1 M) D^-1 r = D^-1/2
        q(N) D^-1/2 r with D the diagonal of M (Handle.jacobi, which raises on a diagonal that is not
        positive) and N = D^-1/2 M D^-1/2; [lo, hi] encloses N's spectrum.  hi=None:
        gershgorin_jacobi(A, shift)[1], the bound of the symmetric form (2 on a five-point stencil
        whatever the coefficient; the Gershgorin bound of D^-1 M is useless on a varying diagonal);
        lo=None: cheb_precond_lo(degree, hi).  For an operator whose diagonal varies AND whose stencil
        is ill conditioned -- variable-coefficient diffusion, a heat step with a varying mass, a graph
        Laplacian plus a shift -- where Jacobi still pays the grid's condition number and the plain
        polynomial is harmful: about Jacobi's SpMMs in degree + 1 times fewer iterations.  Where
        Jacobi alone already leaves a small condition number it gains nothing.  work is then 8 n b
        elements (CHEB_JACOBI_PCG_WORK_BLOCKS); n_spmm as above.  The dict carries
        precond="jacobi-chebyshev", precond_degree and precond_bounds=(lo, hi).

        method="minres" (lz_minres_solve, b <= 64): MINRES, for a symmetric A + shift I that may be
        indefinite (a Helmholtz-type operator, a saddle-point block, A - sigma I at a sigma inside the
        spectrum); the columns in lock step, each by its own scalars, as method="columns".  Same
        arguments and defaults; no preconditioner (a MINRES preconditioner must be positive definite,
        and Jacobi of an indefinite operator is not): precond raises.  The solution runs one pass
        behind the Lanczos step, so a column that takes k steps runs k + 1 passes; iterations counts
        the passes and n_spmm = iterations + 2 + restarts.  work is 5 n b elements
        (MINRES_WORK_BLOCKS), and the device holds 7 blocks.  est is the recurrence's last |phibar| /
        |B_c|, which never grows within a phase.  Status 2 (MINRES_BREAKDOWN) is a breakdown: a scalar
        that is not finite (a NaN in B_c) or gamma = 0 (A + shift I singular on this Krylov space),
        X_c untouched from then on.  The iterations grow as sigma nears an eigenvalue; a singular
        inconsistent system ends with status 1 or 2.  The dict carries method: "minres".

        Returns a dict: X; iters, status (0 met tol on the measured residual, 1 iterations or
        restarts spent, 2 not positive definite), converged (status == 0), resid (measured), est
        (the recurrence's last value) -- NumPy arrays of b entries; restarts, n_spmm, iterations;
        with a preconditioner also precond ("jacobi", "diagonal", "chebyshev" or "jacobi-chebyshev"; without one the dict is the one
        it always was, so out.get("precond") is None); with method="block" also fallback (0 / 1)
        and stop (BCG_* reason of the last stop)."""
        torch = _torch()
        if method not in ("columns", "block", "minres"):
            raise LanczosError('solve: method is "columns", "block" or "minres"')
        if precond is not None and method != "columns":
            raise LanczosError(f'solve: method="{method}" takes no preconditioner')
        n, b = self._blocks("solve", A, B)
        dinv, kind, cheb = None, None, None
        if isinstance(precond, ChebPrecond) or (isinstance(precond, str) and precond in ("chebyshev",
                                                                                         "jacobi-chebyshev")):
            cp = ChebPrecond(jacobi=precond == "jacobi-chebyshev") if isinstance(precond, str) else precond
            if cp.jacobi:
                dinv = self.jacobi(A, shift)
                hi = gershgorin_jacobi(A, shift)[1] if cp.hi is None else float(cp.hi)
            else:
                hi = gershgorin(A)[1] + float(shift) if cp.hi is None else float(cp.hi)
            lo = cheb_precond_lo(cp.degree, hi) if cp.lo is None else float(cp.lo)
            cheb, kind = _cheb_precond((cp.degree, lo, hi)), "jacobi-chebyshev" if cp.jacobi else "chebyshev"
        elif isinstance(precond, str):
            if precond != "jacobi":
                raise LanczosError('solve: precond is None, "jacobi", "chebyshev", "jacobi-chebyshev", a ChebPrecond or '
                                   'a 1-D tensor of n elements')
            dinv, kind = self.jacobi(A, shift), "jacobi"
        elif precond is not None:
            dinv, kind = precond, "diagonal"
            if not torch.is_tensor(dinv) or dinv.dim() != 1 or dinv.numel() != n or dinv.dtype != A.val.dtype \
                    or not dinv.is_contiguous() or dinv.device != B.device:
                raise LanczosError("solve: precond is a contiguous 1-D device tensor of n elements of A's dtype")
        if method == "block" and b > BCG_MAX_B:
            raise LanczosError(f'solve: method="block" takes b <= {BCG_MAX_B}')
        f64 = A.val.dtype == torch.float64
        tol = (1e-10 if f64 else 1e-4) if tol is None else float(tol)
        max_iter = min(10 * n, 10000) if max_iter is None else int(max_iter)
        if X0 is None:
            X = torch.zeros_like(B)
        else:
            self._blocks("solve", A, B, X0)
            X = X0.clone()
        blocks = MINRES_WORK_BLOCKS if method == "minres" \
            else CHEB_JACOBI_PCG_WORK_BLOCKS if cheb is not None and dinv is not None \
            else CHEB_PCG_WORK_BLOCKS if cheb is not None else 4 if dinv is None else PCG_WORK_BLOCKS
        work = self._work4("solve", work, n, b, B, blocks)
        if check_every is not None and check_every < 1:
            raise LanczosError("solve: check_every >= 1")
        opts = CgOpts(tol, max_iter, 0 if check_every is None else int(check_every), int(max_restarts))
        iters, status = np.zeros(b, np.int32), np.zeros(b, np.int32)
        resid, est, info = np.zeros(b), np.zeros(b), np.zeros(3, np.int32)
        args = (self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b, float(shift))
        tail = (_ptr(B), _ptr(X), _ptr(work), ctypes.addressof(opts), _p(iters), _p(status), _p(resid), _p(est))
        if method == "block":
            info = np.zeros(5, np.int32)
            _check(self.L.lz_bcg_solve(*args, *tail, _p(info)), "lz_bcg_solve")
        elif method == "minres":
            _check(self.L.lz_minres_solve(*args, *tail, _p(info)), "lz_minres_solve")
        elif cheb is not None and dinv is not None:
            _check(self.L.lz_pcg_cheb_jacobi_solve(*args, ctypes.addressof(cheb), _ptr(dinv), *tail, _p(info)),
                   "lz_pcg_cheb_jacobi_solve")
        elif dinv is not None:
            _check(self.L.lz_pcg_solve(*args, _ptr(dinv), *tail, _p(info)), "lz_pcg_solve")
        elif cheb is not None:
            _check(self.L.lz_pcg_cheb_solve(*args, ctypes.addressof(cheb), *tail, _p(info)), "lz_pcg_cheb_solve")
        else:
            _check(self.L.lz_cg_solve(*args, *tail, _p(info)), "lz_cg_solve")
        out = {"X": X, "iters": iters, "status": status, "converged": status == 0, "resid": resid, "est": est,
               "iterations": int(info[0]), "restarts": int(info[1]), "n_spmm": int(info[2])}
        if method == "block":
            out.update(fallback=int(info[3]), stop=int(info[4]))
        elif method == "minres":
            out["method"] = "minres"
        elif dinv is not None and cheb is None:
            out["precond"] = kind
        elif cheb is not None:
            out.update(precond=kind, precond_degree=cheb.degree, precond_bounds=(cheb.lo, cheb.hi))
        return out

    @staticmethod
    def _work4(what: str, work, n: int, b: int, like, blocks: int = 4):
        torch = _torch()
        if work is None:
            return torch.empty(blocks * n * b, dtype=like.dtype, device=like.device)
        if work.dim() != 1 or not work.is_contiguous() or work.numel() < blocks * n * b or work.dtype != like.dtype:
            raise LanczosError(f"{what}: work is a flat contiguous tensor of {blocks}*n*b elements of B's dtype")
        return work

    def mscg_update(self, coef, live, R, W, S, P, X, rr=None):
        """The row-local pass of one multi-shift conjugate-gradient step (lz_mscg_update): for every
        shift k with live[k] != 0 and a_k != 0, P_k = zeta_k R + b_k P_k and X_k += a_k P_k (the old R,
        each element finished as one fma), then cg_update's S = W + beta S, R -= alpha S and rr.  coef:
        (2 + 3 s) b fp64 on the device, [alpha | beta | zeta_0 | a_0 | b_0 | zeta_1 | ...]; live: s
        int32 on the device; R, W (read only), S: (n, b); P, X: (s, n, b); all contiguous, of one
        dtype, pairwise distinct, s <= MSCG_MAX_SHIFTS.  A shift that is not live is neither read nor
        written; a_k == 0 leaves its column of P_k and X_k bit for bit.  Returns rr."""
        torch = _torch()
        n, b = R.shape
        for t in (R, W, S):
            if tuple(t.shape) != (n, b) or t.dtype != R.dtype or not t.is_contiguous():
                raise LanczosError("mscg_update: R, W, S (n, b) contiguous (ld = b), of one dtype")
        s = P.shape[0] if P.dim() == 3 else -1
        for t in (P, X):
            if t.dim() != 3 or tuple(t.shape) != (s, n, b) or t.dtype != R.dtype or not t.is_contiguous():
                raise LanczosError("mscg_update: P, X (s, n, b) contiguous, of R's dtype")
        if not 1 <= s <= MSCG_MAX_SHIFTS:
            raise LanczosError(f"mscg_update: 1 <= s <= {MSCG_MAX_SHIFTS}")
        if coef.dtype != torch.float64 or not coef.is_contiguous() or coef.numel() != (2 + 3 * s) * b:
            raise LanczosError("mscg_update: coef is a contiguous fp64 tensor of (2 + 3 s) b elements")
        if live.dtype != torch.int32 or not live.is_contiguous() or live.numel() != s:
            raise LanczosError("mscg_update: live is a contiguous int32 tensor of s elements")
        if rr is None:
            rr = torch.empty(b, dtype=torch.float64, device=R.device)
        if rr.dtype != torch.float64 or not rr.is_contiguous() or rr.numel() != b:
            raise LanczosError("mscg_update: rr is a contiguous fp64 tensor of b elements")
        _check(self.L.lz_mscg_update(self.ptr, n, b, _dt(R), s, _ptr(coef), _ptr(live), _ptr(R), _ptr(W), _ptr(S),
                                     _ptr(P), _ptr(X), _ptr(rr)), "lz_mscg_update")
        return rr

    def solve_shifts(self, A: CsrDevice, B, shifts, tol: Optional[float] = None, max_iter: Optional[int] = None,
                     check_every: Optional[int] = None, max_restarts: int = 3, work=None) -> dict:
        """Solve (A + shifts[k] I) X_k = B for every shift by multi-shift conjugate gradients
        (lz_mscg_solve): one SpMM per iteration for all s <= MSCG_MAX_SHIFTS shifts and b <= 64
        columns.  Conjugate gradients run on the smallest shift, the seed; every other shift takes
        its solution from the seed's residual by three scalars per column.  Then every shift's
        residual is measured and a shift that missed tol is polished by solve's plain conjugate
        gradients (the finishing phase), so status 0 is a measured residual as in solve.
        tol, max_iter, check_every, max_restarts: solve's, with its defaults.  work: (3 + s) n b
        elements, [R | W | S | P_0 .. P_{s-1}].  No preconditioner and no start block; the seed's
        operator must be positive definite for the shared phase to help.
        Returns a dict: X (s, n, b) in the caller's shift order; iters (the shared phase's),
        finish_iters (the polish's), status, converged, resid (the finishing phase's), est (the shared
        phase's) as (s, b) arrays; iterations (shared, enqueued), n_spmm (all), finished (pairs with
        finish_iters > 0), restarts (the finishing phase's) and seed (the index of the smallest
        shift)."""
        torch = _torch()
        n, b = self._blocks("solve_shifts", A, B)
        try:
            sh = np.ascontiguousarray(np.asarray(shifts, np.float64).reshape(-1))
        except (TypeError, ValueError):
            raise LanczosError("solve_shifts: shifts is a sequence of numbers")
        s = int(sh.size)
        if not 1 <= s <= MSCG_MAX_SHIFTS:
            raise LanczosError(f"solve_shifts: 1 <= len(shifts) <= {MSCG_MAX_SHIFTS}")
        f64 = A.val.dtype == torch.float64
        tol = (1e-10 if f64 else 1e-4) if tol is None else float(tol)
        max_iter = min(10 * n, 10000) if max_iter is None else int(max_iter)
        work = self._work4("solve_shifts", work, n, b, B, 3 + s)
        if check_every is not None and check_every < 1:
            raise LanczosError("solve_shifts: check_every >= 1")
        opts = CgOpts(tol, max_iter, 0 if check_every is None else int(check_every), int(max_restarts))
        X = torch.empty(s, n, b, dtype=B.dtype, device=B.device)
        iters, fin, status = (np.zeros((s, b), np.int32) for _ in range(3))
        resid, est, info = np.zeros((s, b)), np.zeros((s, b)), np.zeros(4, np.int32)
        _check(self.L.lz_mscg_solve(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b, s,
                                    _p(sh), _ptr(B), _ptr(X), _ptr(work), ctypes.addressof(opts), _p(iters), _p(fin),
                                    _p(status), _p(resid), _p(est), _p(info)), "lz_mscg_solve")
        rounded = sh.astype(np.float64 if f64 else np.float32)
        return {"X": X, "iters": iters, "finish_iters": fin, "status": status, "converged": status == 0,
                "resid": resid, "est": est, "iterations": int(info[0]), "n_spmm": int(info[1]),
                "finished": int(info[2]), "restarts": int(info[3]), "seed": int(np.argmin(rounded))}

    def spectral_moments(self, A: CsrDevice, n_moments: int = 257, probes: Optional[int] = None,
                         b: Optional[int] = None, bounds=None, pad: float = 0.01, seed: int = 0,
                         X0=None) -> KpmMoments:
        """Chebyshev moments of the symmetric operator A by the kernel polynomial method: K =
        ceil((n_moments - 1) / 2) three-term SpMMs per block of b random +-1 probe columns give
        2K+1 moments per probe; KpmMoments.count / .density read eigenvalue counts and the
        density of states off them, for any number of intervals.
        b: the probe block (default the 128-byte row of A's dtype: 16 fp64, 32 fp32); probes: a
        multiple of b (default b).  bounds: an enclosure (lo, hi) of the spectrum, default
        gershgorin(A) (one copy of the CSR arrays to the host); each end is moved out by pad x
        the width.  An eigenvalue outside the widened bounds makes the recurrence diverge:
        non-finite dots raise LanczosError.  The probes are drawn on the device from
        torch.Generator(seed), block by block, unless X0 (n x probes) is given.  One
        cheb_moments call and one copy of its dots to the host per block."""
        torch = _torch()
        n = A.n
        if b is None:
            b = 16 if A.dtype == LZ_F64 else 32
        if X0 is not None:
            probes = X0.shape[1]
        elif probes is None:
            probes = b
        if n_moments < 2 or b < 1 or probes < b or probes % b:
            raise LanczosError("spectral_moments: n_moments >= 2, probes a positive multiple of b")
        if X0 is not None and (X0.shape[0] != n or X0.dtype != A.val.dtype):
            raise LanczosError("spectral_moments: X0 is n x probes, of A's dtype")
        K = -(-(n_moments - 1) // 2)
        lo, hi = gershgorin(A) if bounds is None else (float(bounds[0]), float(bounds[1]))
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and pad >= 0):
            raise LanczosError(f"spectral_moments: bounds ({lo}, {hi}) must be finite with lo < hi, pad >= 0")
        lo, hi = lo - pad * (hi - lo), hi + pad * (hi - lo)
        dev, dt = A.val.device, A.val.dtype
        gen = None
        if X0 is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
        work = torch.empty(3 * n * b, dtype=dt, device=dev)
        dots = torch.empty(K + 1, 2, b, dtype=torch.float64, device=dev)
        mu = np.empty((2 * K + 1, probes))
        for j in range(probes // b):
            if X0 is None:
                Xb = (torch.randint(0, 2, (n, b), generator=gen, device=dev, dtype=torch.int8) * 2 - 1).to(dt)
            else:
                Xb = X0[:, j * b:(j + 1) * b].contiguous()
            raw = _f64(self.cheb_moments(A, Xb, K, lo, hi, work=work, dots=dots))
            if not np.isfinite(raw).all():
                raise LanczosError(f"spectral_moments: non-finite moments -- the bounds ({lo}, {hi}) do not enclose "
                                   "the operator's spectrum")
            mu[:, j * b:(j + 1) * b] = kpm_moments(raw)
        return KpmMoments(n, lo, hi, mu, K * (probes // b))

    def eigcount(self, A: CsrDevice, a: float, b: float, /, **kw):
        """(estimate, stderr) of the number of eigenvalues of A in [a, b]:
        spectral_moments(A, **kw).count(a, b).  a and b are positional only, so that kw may
        carry spectral_moments' own b (the probe block)."""
        return self.spectral_moments(A, **kw).count(a, b)

    def _work(self, what: str, work, n: int, b: int, like):
        if work.dim() != 1 or not work.is_contiguous() or work.numel() < 2 * n * b or work.dtype != like.dtype:
            raise LanczosError(f"{what}: work is a flat contiguous tensor of 2*n*b elements of the solve's dtype")

    def cheb_apply(self, A: CsrDevice, filt, X, Y, work):
        """Y = p(A) X with p the scaled Chebyshev filter filt = (degree, lo, hi, ref)
        (lz_cheb_apply): damped on [lo, hi], 1 at ref.  work: flat, 2*n*b elements; X is only
        read."""
        n, b = self._blocks("cheb_apply", A, X, Y)
        self._work("cheb_apply", work, n, b, X)
        f = _cheb(filt)
        _check(self.L.lz_cheb_apply(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                    ctypes.addressof(f), _ptr(X), _ptr(Y), _ptr(work)), "lz_cheb_apply")
        return Y

    def cheb_series_apply(self, A: CsrDevice, series, X, Y, work):
        """Y = sum_k gamma_k T_k((A - c0) / e) X for series = (degree, lo, hi, gamma), [lo, hi] =
        [c0 - e, c0 + e] enclosing A's spectrum and gamma the degree + 1 coefficients
        (cheb_window makes a window's), by Clenshaw's recurrence: degree SpMMs
        (lz_cheb_series_apply).  work: flat, 2*n*b elements; X is only read."""
        n, b = self._blocks("cheb_series_apply", A, X, Y)
        self._work("cheb_series_apply", work, n, b, X)
        degree, lo, hi, gamma = self._series("cheb_series_apply", series)
        _check(self.L.lz_cheb_series_apply(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                           degree, lo, hi, _p(gamma), _ptr(X), _ptr(Y), _ptr(work)),
               "lz_cheb_series_apply")
        return Y

    def _normal(self, what: str, normal, n: int, b: int, like):
        """(P, Pt, work) of a normal-operator call on n x b blocks: P (p, n), Pt (n, p) its
        transpose, work flat with p*b elements of the blocks' dtype."""
        P, Pt, work = normal
        if P.n_cols != n or Pt.n != n or Pt.n_cols != P.n or P.nnz != Pt.nnz or P.val.dtype != like.dtype \
                or Pt.val.dtype != like.dtype:
            raise LanczosError(f"{what}: P (p, n) and Pt (n, p) its transpose, of the blocks' dtype, n the blocks' rows")
        if work is None or work.dim() != 1 or not work.is_contiguous() or work.numel() < P.n * b \
                or work.dtype != like.dtype:
            raise LanczosError(f"{what}: work is a flat contiguous tensor of p*b elements of the solve's dtype")
        return P, Pt, work

    @staticmethod
    def _series(what: str, series):
        """(degree, lo, hi, gamma) of a Chebyshev series, gamma as degree + 1 contiguous host doubles."""
        degree, lo, hi, gamma = series
        gamma = np.ascontiguousarray(gamma, np.float64)
        if int(degree) < 1 or gamma.ndim != 1 or gamma.size != int(degree) + 1:
            raise LanczosError(f"{what}: series = (degree, lo, hi, gamma) with degree >= 1 and degree + 1 coefficients")
        return int(degree), float(lo), float(hi), gamma

    @staticmethod
    def _inverse(what: str, inverse, work, n: int, b: int, like):
        """(Inverse, InverseInfo) of inverse = (sigma, inner, tol, max_iter, info) on n x b blocks:
        inner "minres", "columns" or "block"; max_iter None: min(10 n, 10000), solve's default;
        info an InverseInfo that the call accumulates into; work flat, MINRES_WORK_BLOCKS*n*b
        elements of the blocks' dtype."""
        sigma, inner, tol, max_iter, info = inverse
        if inner not in INNER_METHODS:
            raise LanczosError(f'{what}: inner is "minres", "columns" or "block"')
        if not isinstance(info, InverseInfo):
            raise LanczosError(f"{what}: inverse = (sigma, inner, tol, max_iter, info) with info an InverseInfo")
        if inner == "block" and b > BCG_MAX_B:
            raise LanczosError(f'{what}: inner="block" takes b <= {BCG_MAX_B}')
        k = MINRES_WORK_BLOCKS
        if work is None or work.dim() != 1 or not work.is_contiguous() or work.numel() < k * n * b \
                or work.dtype != like.dtype:
            raise LanczosError(f"{what}: work is a flat contiguous tensor of {k}*n*b elements of the solve's dtype")
        max_iter = min(10 * n, 10000) if max_iter is None else int(max_iter)
        return Inverse(float(sigma), INNER_METHODS[inner], CgOpts(float(tol), max_iter, 0, 3)), info

    def _reorth_op(self, what: str, A, n: int, b: int, like, filt, work, normal, series=None,
                   inverse=None) -> "_ReorthOp":
        """The operator of a kept-basis solve (A, p(A), Pt (P .), a Chebyshev series s(A) or the
        inverse (A - sigma I)^-1: block_lanczos_reorth's docstring), validated, as the ABI function
        lz_<what>[_cheb | _normal | _series | _inverse] with the arguments that differ between
        the five."""
        csr = lambda M: (_ptr(M.row_ptr), _ptr(M.col), _ptr(M.val))
        if inverse is not None:
            if filt is not None or normal is not None or series is not None:
                raise LanczosError(f"{what}: inverse= is mutually exclusive with filt=, normal= and series=")
            inv, info = self._inverse(what, inverse, work, n, b, like)
            return _ReorthOp(f"lz_{what}_inverse", (n, A.nnz, *csr(A), A.dtype),
                             (ctypes.addressof(inv), _ptr(work), ctypes.addressof(info)), inv)
        if series is not None:
            if filt is not None or normal is not None:
                raise LanczosError(f"{what}: series= is mutually exclusive with filt= and normal=")
            self._work(what, work, n, b, like)
            degree, lo, hi, gamma = self._series(what, series)
            return _ReorthOp(f"lz_{what}_series", (n, A.nnz, *csr(A), A.dtype), (degree, lo, hi, _p(gamma), _ptr(work)),
                             gamma)
        if normal is not None:
            if filt is not None:
                raise LanczosError(f"{what}: normal= and filt= are mutually exclusive")
            P, Pt, nwork = self._normal(what, normal, n, b, like)
            return _ReorthOp(f"lz_{what}_normal", (n, P.n, P.nnz, *csr(P), *csr(Pt), P.dtype), (_ptr(nwork),), None)
        head = (n, A.nnz, *csr(A), A.dtype)
        if filt is None:
            return _ReorthOp(f"lz_{what}", head, (), None)
        self._work(what, work, n, b, like)
        f = _cheb(filt)
        return _ReorthOp(f"lz_{what}_cheb", head, (ctypes.addressof(f), _ptr(work)), f)

    def normal_apply(self, P: CsrDevice, Pt: CsrDevice, X, Y, work):
        """Y = Pt (P X) (lz_normal_apply): P (p, n), Pt = P.transpose(handle), X / Y (n, b)
        contiguous and distinct, work flat with p*b elements.  X is only read."""
        n, b = X.shape
        if tuple(Y.shape) != (n, b) or not X.is_contiguous() or not Y.is_contiguous() or Y.dtype != X.dtype:
            raise LanczosError("normal_apply: X and Y (n, b) contiguous (ld = b), one dtype")
        self._normal("normal_apply", (P, Pt, work), n, b, X)
        _check(self.L.lz_normal_apply(self.ptr, n, P.n, P.nnz, _ptr(P.row_ptr), _ptr(P.col), _ptr(P.val),
                                      _ptr(Pt.row_ptr), _ptr(Pt.col), _ptr(Pt.val), P.dtype, b, _ptr(X), _ptr(Y),
                                      _ptr(work)), "lz_normal_apply")
        return Y

    def inverse_apply(self, A: CsrDevice, inverse, X, Y, work):
        """Y = (A - sigma I)^-1 X by one inner solve from a zero start block (lz_inverse_apply),
        the operator line of eigsh(sigma=...): inverse = (sigma, inner, tol, max_iter, info) with
        inner "minres" (any sigma), "columns" or "block" (conjugate gradients: A - sigma I
        positive definite), tol the relative residual of a column, info an InverseInfo the call
        accumulates into.  X (read only), Y (n, b) contiguous and distinct; work flat,
        MINRES_WORK_BLOCKS*n*b elements.  A column that misses tol is counted in info.not_met, not
        raised.  Synchronises the stream."""
        n, b = self._blocks("inverse_apply", A, X, Y)
        inv, info = self._inverse("inverse_apply", inverse, work, n, b, X)
        _check(self.L.lz_inverse_apply(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                       _ptr(X), _ptr(Y), ctypes.addressof(inv), _ptr(work), ctypes.addressof(info)),
               "lz_inverse_apply")
        return Y

    def to_row_major(self, Xcm, Y):
        """Y (rows, b) row-major <- the column-major block viewed as Xcm (b, ld) (ld >= rows)."""
        b, ld = Xcm.shape
        rows = Y.shape[0]
        _check(self.L.lz_to_row_major(self.ptr, rows, b, _dt(Xcm), _ptr(Xcm), ld, _ptr(Y)), "lz_to_row_major")
        return Y

    def to_col_major(self, X, Ycm):
        """The column-major block viewed as Ycm (b, ld) (ld >= rows) <- X (rows, b) row-major, contiguous."""
        rows, b = X.shape
        if not X.is_contiguous() or Ycm.shape[0] != b or (b > 1 and Ycm.stride(1) != 1):
            raise LanczosError("to_col_major: X (rows, b) contiguous, Ycm (b, ld) with unit inner stride")
        ld = Ycm.stride(0) if b > 1 else Ycm.shape[1]
        _check(self.L.lz_to_col_major(self.ptr, rows, b, _dt(X), _ptr(X), _ptr(Ycm), ld), "lz_to_col_major")
        return Ycm

    def spmv(self, A: CsrDevice, x, y):
        _check(self.L.lz_csr_spmv(self.ptr, A.n, A.n_cols, A.nnz, _ptr(A.row_ptr), _ptr(A.col),
                                  _ptr(A.val), A.dtype, _ptr(x), _ptr(y)), "lz_csr_spmv")
        return y

    def mm_tt(self, W, R):
        """R = W^T W (mm_tt_cublas, utils/lib_utils.hpp:102-123)."""
        n, b = W.shape
        _check(self.L.lz_gram(self.ptr, n, b, _dt(W), _ptr(W), W.stride(0), _ptr(R)), "lz_gram")
        return R

    def mm_tt2(self, W, Q, R):
        """R = 0.5 (W^T Q + Q^T W) (mm_tt2_cublas, lib_utils.hpp:164-202)."""
        n, b = W.shape
        if Q.shape != W.shape or (n > 1 and Q.stride(0) != W.stride(0)):
            raise LanczosError("mm_tt2: W and Q must have the same shape and row stride (one ld for both)")
        _check(self.L.lz_sym_cross_gram(self.ptr, n, b, _dt(W), _ptr(W), _ptr(Q), W.stride(0), _ptr(R)),
               "lz_sym_cross_gram")
        return R

    def mm_ts(self, beta: float, alpha: float, Q, S, W):
        """W = beta W + alpha Q S (mm_cublas(beta, alpha, Q, S, W), lib_utils.hpp:28-51)."""
        n, b = Q.shape
        if W.shape != Q.shape or (n > 1 and Q.stride(0) != W.stride(0)):
            raise LanczosError("mm_ts: Q and W must have the same shape and row stride (one ld for both)")
        _check(self.L.lz_tsmm(self.ptr, n, b, _dt(Q), beta, alpha, _ptr(Q), _ptr(S), _ptr(W), W.stride(0)),
               "lz_tsmm")
        return W

    def sqrtm(self, G, beta, beta_inv, eigval=None):
        """beta = sqrtm(G), beta_inv = inverse (sqrtm_cusolver, lib_utils.hpp:721-745)."""
        b = G.shape[0]
        _check(self.L.lz_sqrtm_pair(self.ptr, b, _dt(G), _ptr(G), _ptr(beta), _ptr(beta_inv), _ptr(eigval)),
               "lz_sqrtm_pair")

    def copy_row_to_vector(self, lc: int, start: int, Q, q, layout: int = LZ_ROW_MAJOR):
        """q[start : start + b] = row lc of Q: (rows, b) row-major, or the
        column-major block viewed as (b, ld) when layout=LZ_COL_MAJOR."""
        b = Q.shape[1] if layout == LZ_ROW_MAJOR else Q.shape[0]
        _check(self.L.lz_copy_row(self.ptr, b, _dt(Q), _ptr(Q), Q.stride(0), layout, lc, _ptr(q), start),
               "lz_copy_row")

    def block_lanczos_blas(self, A: CsrDevice, B, m: int, lc: int, q, alpha, beta, Q0, Q1, W,
                           fused: bool = True):
        """block_lanczos_blas (methods/block_lanczos.hpp:88-167).  q[m*b], alpha[m,b,b],
        beta[m+1,b,b] device tensors are written in place."""
        n, b = B.shape
        fn = self.L.lz_block_lanczos if fused else self.L.lz_block_lanczos_unfused
        _check(fn(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b, m, lc,
                  _ptr(B), _ptr(q), _ptr(alpha), _ptr(beta), _ptr(Q0), _ptr(Q1), _ptr(W)),
               "lz_block_lanczos")

    # --- kept basis: panel kernels, reorthogonalised solve, Ritz vectors -----
    @staticmethod
    def _panel(V, vstride: int, n: int, b: int, k: int):
        """A basis panel is a flat tensor: block j = V[j*vstride : j*vstride + n*b] viewed (n, b)."""
        if V.dim() != 1 or not V.is_contiguous() or V.numel() < (k - 1) * vstride + n * b:
            raise LanczosError("a basis panel is a flat contiguous tensor of at least (k-1)*vstride + n*b elements")

    def panel_gram(self, V, vstride: int, k: int, W, C):
        """C (k, b, b) = [V_j^T W for j < k] over the first k blocks of the panel V (lz_panel_gram)."""
        n, b = W.shape
        self._panel(V, vstride, n, b, max(k, 1))
        if not W.is_contiguous() or not C.is_contiguous() or C.numel() < k * b * b or C.dtype != W.dtype \
                or V.dtype != W.dtype:
            raise LanczosError("panel_gram: W (n, b) and C (k, b, b) contiguous, one dtype")
        _check(self.L.lz_panel_gram(self.ptr, n, b, k, _dt(W), _ptr(V), vstride, _ptr(W), _ptr(C)), "lz_panel_gram")
        return C

    def panel_apply(self, beta: float, alpha: float, V, vstride: int, k: int, S, W):
        """W = beta W + alpha sum_{j<k} V_j S_j, S (k, b, b) on the device (lz_panel_apply)."""
        n, b = W.shape
        self._panel(V, vstride, n, b, max(k, 1))
        if not W.is_contiguous() or not S.is_contiguous() or S.numel() < k * b * b or S.dtype != W.dtype \
                or V.dtype != W.dtype:
            raise LanczosError("panel_apply: W (n, b) and S (k, b, b) contiguous, one dtype")
        _check(self.L.lz_panel_apply(self.ptr, n, b, k, _dt(W), beta, alpha, _ptr(V), vstride, _ptr(S), _ptr(W)),
               "lz_panel_apply")
        return W

    def block_lanczos_reorth(self, A: CsrDevice, B, m: int, lc: int, q, alpha, beta, V, vstride: int, W,
                             passes: int = 2, filt=None, work=None, normal=None, series=None, inverse=None):
        """Block Lanczos on a kept basis with `passes` rounds of full reorthogonalisation
        per step (lz_block_lanczos_reorth).  q[m*b], alpha[m,b,b], beta[m+1,b,b] (beta[m]
        = the true beta_m), the panel V (m blocks) and W (the final residual) are written
        in place.  filt = (degree, lo, hi, ref) with work (flat, 2*n*b elements): the same
        solve on the Chebyshev-filtered operator p(A) (lz_block_lanczos_reorth_cheb).
        normal = (P, Pt, work) with P (p, n), Pt its transpose and work flat with p*b elements:
        the same solve on G = P^T P (lz_block_lanczos_reorth_normal); A is not used then (None)
        and filt must be None.  series = (degree, lo, hi, gamma) with work as for filt: the
        same solve on the Chebyshev series sum_k gamma_k T_k((A - c0) / e) of cheb_series_apply
        (lz_block_lanczos_reorth_series); filt and normal must be None.  inverse = (sigma, inner,
        tol, max_iter, info) with work flat, MINRES_WORK_BLOCKS*n*b elements: the same solve on
        (A - sigma I)^-1, every operator line one inner solve as inverse_apply runs it
        (lz_block_lanczos_reorth_inverse); filt, normal and series must be None.  Such a cycle
        synchronises the stream at every step."""
        n, b = B.shape
        self._panel(V, vstride, n, b, max(m, 1))
        op = self._reorth_op("block_lanczos_reorth", A, n, b, W, filt, work, normal, series, inverse)
        _check(getattr(self.L, op.name)(self.ptr, *op.head, b, m, lc, _ptr(B), _ptr(q), _ptr(alpha), _ptr(beta),
                                        _ptr(V), vstride, _ptr(W), passes, *op.tail), op.name)

    def ritz_vectors(self, V, vstride: int, S, X, n: int, b: int):
        """X = [V_0 .. V_{m-1}] S: the Ritz vectors of host coefficients S ((m*b, nev),
        ritz_pairs) into a second block-major panel X of ceil(nev / b) blocks (same
        vstride, n and b as V), chunk c holding columns [c*b, (c+1)*b) of the product as
        an (n, b) block; a last chunk narrower than b is zero-padded.  One lz_panel_apply
        (beta = 0) per chunk.  V and X are contiguous tensors of any shape (flat, or
        (blocks, vstride))."""
        torch = _torch()
        S = np.ascontiguousarray(S, np.float64)
        mb, nev = S.shape
        if not V.is_contiguous() or not X.is_contiguous():
            raise LanczosError("ritz_vectors: V and X must be contiguous")
        V, X = V.view(-1), X.view(-1)
        if mb % b:
            raise LanczosError("ritz_vectors: S must have m*b rows")
        m, nch = mb // b, -(-nev // b)
        self._panel(V, vstride, n, b, m)
        self._panel(X, vstride, n, b, nch)
        Sd = torch.from_numpy(_pack_chunks(S, m, b)).to(device=V.device, dtype=V.dtype)
        for c in range(nch):
            Xc = X[c * vstride:c * vstride + n * b].view(n, b)
            self.panel_apply(0.0, 1.0, V, vstride, m, Sd[c], Xc)
        return X

    def panel_compress(self, V, vstride: int, k: int, r: int, Z, n: Optional[int] = None):
        """In place: block c < r of the panel V = sum_{j<k} V_j Z[c][j], Z (r, k, b, b) on the
        device (lz_panel_compress; b is Z's).  Blocks r .. k-1 and the padding between blocks
        are not written.  n: rows of a block; default vstride / b, an unpadded panel."""
        if Z.dim() != 4 or Z.shape[2] != Z.shape[3] or not Z.is_contiguous() or Z.dtype != V.dtype \
                or (k >= 1 and r >= 1 and tuple(Z.shape[:2]) != (r, k)):
            raise LanczosError("panel_compress: Z (r, k, b, b) contiguous, of the panel's dtype")
        b = Z.shape[2]
        if n is None:
            if vstride % b:
                raise LanczosError("panel_compress: pass n for a padded panel (vstride is no multiple of b)")
            n = vstride // b
        self._panel(V, vstride, n, b, max(k, 1))
        _check(self.L.lz_panel_compress(self.ptr, n, b, k, r, _dt(V), _ptr(V), vstride, _ptr(Z)), "lz_panel_compress")
        return V

    def block_lanczos_reorth_resume(self, A: CsrDevice, r: int, m: int, lc: int, sigma, q, alpha, beta, V,
                                    vstride: int, W, passes: int = 2, filt=None, work=None, normal=None,
                                    series=None, inverse=None):
        """Steps r .. m-1 of block_lanczos_reorth on a thick-restarted basis
        (lz_block_lanczos_reorth_resume): blocks 0 .. r-1 of V hold the kept Ritz blocks
        (panel_compress), W the previous cycle's residual, sigma (r, b, b) the device copy of
        restart_coeffs' sigma.  Writes alpha[r:], beta[r:], q[r*b:], blocks r .. m-1 and W.
        filt, work, normal, series, inverse: as block_lanczos_reorth (the same operator for every
        cycle of a solve)."""
        n, b = W.shape
        self._panel(V, vstride, n, b, max(m, 1))
        if not sigma.is_contiguous() or sigma.numel() < max(r, 0) * b * b or sigma.dtype != W.dtype \
                or V.dtype != W.dtype or not W.is_contiguous():
            raise LanczosError("block_lanczos_reorth_resume: W (n, b) and sigma (r, b, b) contiguous, one dtype")
        op = self._reorth_op("block_lanczos_reorth_resume", A, n, b, W, filt, work, normal, series, inverse)
        _check(getattr(self.L, op.name)(self.ptr, *op.head, b, r, m, lc, _ptr(sigma), _ptr(q), _ptr(alpha),
                                        _ptr(beta), _ptr(V), vstride, _ptr(W), passes, *op.tail), op.name)

    def eigsh(self, A: CsrDevice, nev: int, which: str = "largest", b: int = 16, m: Optional[int] = None,
              keep: Optional[int] = None, tol: float = 1e-10, max_cycles: int = 100, B=None, lc: int = 0,
              passes: int = 2, filter_degree: Optional[int] = None, cut: Optional[float] = None,
              sigma: Optional[float] = None, inner: str = "minres", inner_tol: Optional[float] = None,
              inner_max_iter: Optional[int] = None):
        """The nev outermost eigenpairs of A by thick-restart block Lanczos in a fixed panel
        of m blocks.  Cycle 1 is block_lanczos_reorth from B (default uniform_B); every later
        cycle keeps the first keep*b Ritz pairs (restart_coeffs), compresses the panel onto
        them in place (panel_compress) and resumes (block_lanczos_reorth_resume).  It stops
        when the nev wanted pairs all have resid <= tol * max|theta| (ritz_pairs_dense; the
        maximum over every Ritz value of T, the cycle's estimate of ||A||_2), or after
        max_cycles cycles (converged = False, no exception).  One more panel_compress
        leaves the nev Ritz vectors in the first ceil(nev / b) blocks of the panel, the last
        zero-padded.  keep * b >= nev, keep <= PANEL_MAX_KEEP, keep < m <= PANEL_MAX_BLOCKS;
        default keep: the smallest with keep * b >= nev + b, clipped to those limits; default
        m: twice that, at least 4.  The solve's precision is A's.  Device memory that scales with n: the
        panel, W and B.  Returns a dict: theta[nev], resid[nev], V (the panel, flat), vstride,
        cycles, n_spmm, converged, history (the largest wanted residual of each cycle), scale
        (the last cycle's max|theta|).

        Limits, in every form: m * b <= n (refused with the other arguments).  A rank-deficient
        block -- a start block with a zero or (nearly) duplicated column, an operator of rank
        below m * b - b, a start block inside an invariant subspace, an exhausted Krylov space --
        raises LanczosError("... is rank deficient ...") naming the start block or the cycle and
        step (rank_ratios against RANK_DELTA_*; host work on the beta blocks already copied back):
        beta^-1 = 1 / sqrt|lambda| would leave the panel neither normalised nor orthogonal.
        Only LanczosError leaves the solve.  Repeated eigenvalues up to multiplicity b come out
        complete; one of multiplicity above b is not guaranteed to.

        filter_degree = d (1 .. 256): the same restart on p(A), a degree-d scaled Chebyshev
        filter, for ends that converge slowly (the smallest eigenvalues of Laplacian-like
        operators).  One unfiltered solve of m blocks gives the Ritz values theta of A (and
        returns at once if it already meets the stop test); p damps [theta[keep*b], g_hi]
        (which = "smallest"; mirrored for "largest"; g: gershgorin(A); cut replaces the
        Ritz-value end) and is 1 at the outermost theta, fixed for the whole solve.  After
        every cycle's compress the first ceil(nev / b) kept blocks are checked on A itself,
        block by block (Rayleigh-Ritz within the block, true residual norms); it stops when
        the nev candidates at the wanted end have residuals <= tol * scale (scale: the
        unfiltered solve's max|theta|).  The dict then also has cols[nev] (the panel column
        of each pair, which need not be the first nev: V is not re-packed), filter = (degree,
        lo, hi, ref), n_steps (Lanczos steps, the unfiltered solve included); resid is the
        measured residual on A, cycles counts the filtered cycles, n_spmm every SpMM
        (bounds, filter steps and checks).  Needs 2 n b more elements of device memory.

        sigma given: the nev eigenpairs nearest sigma, anywhere in the spectrum, by the same restart
        on (A - sigma I)^-1 (shift-and-invert), whose Ritz values nu = 1 / (lambda - sigma) of
        largest magnitude are the wanted ones.  which must stay at its default and filter_degree
        None.  Every operator line is one inner solve of b columns from a zero start (inverse_apply):
        inner = "minres" for any sigma; "columns" or "block" (conjugate gradients) for a sigma
        below the spectrum -- a solve in which a column reports "not positive definite" raises and
        names inner="minres".  inner_tol: the relative residual of an inner column, default
        max(INNER_TOL_FACTOR * tol, INNER_TOL_FLOOR_EPS * eps); inner_max_iter: default min(10 n,
        10000).  An inner column that misses inner_tol does not stop the solve (inner_not_met
        counts it): the stop test is measured on A.  After every cycle's compress ("magnitude"):
        Rayleigh-Ritz on A over the keep kept blocks as eigsh_interval does it (H = Y^T A Y by one
        spmm and one panel_gram per block, eigh on the host, the rotated blocks by panel_apply) with
        the residuals ||A x - lambda x|| of each rotated block from one spmm_resid; the panel is
        not rotated.  Converged when the nev kept pairs nearest sigma have residuals <= tol *
        scale, scale = max(|lo|, |hi|) of gershgorin(A); else max_cycles (converged = False).  One
        panel_compress packs the nev vectors, ordered by |lambda - sigma| ascending.  The dict:
        theta, resid (measured on A), V, vstride, cycles, converged, history, scale as above, and
        sigma, inner, inner_tol, inner_solves, inner_passes, inner_not_met, inner_worst,
        inner_breakdown (the InverseInfo counts), n_steps (Lanczos steps = inner solves), n_spmm
        (every SpMM: the inner solves' and 2 keep per check).  Needs 5 n b more elements of device
        memory.  The cost of an inner solve grows as sigma nears an eigenvalue; there is no
        preconditioner."""
        if sigma is not None:
            if which != "largest":
                raise LanczosError("eigsh: sigma= selects the pairs nearest sigma; which must stay at its default")
            if filter_degree is not None or cut is not None:
                raise LanczosError("eigsh: sigma= and filter_degree= / cut= are mutually exclusive")
            return self._eigsh_sigma(A, nev, float(sigma), b, m, keep, tol, max_cycles, B, lc, passes, inner,
                                     inner_tol, inner_max_iter)
        _which(which)
        if filter_degree is not None and not 1 <= int(filter_degree) <= 256:
            raise LanczosError("eigsh: 1 <= filter_degree <= 256")
        m, r = _restart_sizes("eigsh", "nev", nev, b, m, keep, A.n)
        d = _Restart(self, A, A.n, b, m, r, lc, passes, A.val)
        B = d.start_block(B)
        if filter_degree is not None:
            return self._eigsh_cheb(d, nev, which, tol, max_cycles, B, int(filter_degree), cut)
        d.first(B)
        history = []
        while True:
            theta, S, resid, scale = d.ritz(which)
            theta, S, resid = theta[:nev], S[:, :nev], resid[:nev]
            history.append(float(resid.max()))
            converged = bool(resid.max() <= tol * scale)
            if converged or d.cycles >= max_cycles:
                break
            d.compress(which)
            d.resume()
        d.pack(S, nev)  # the wanted Ritz vectors, in place, into the first ceil(nev / b) blocks
        return dict(theta=theta, resid=resid, V=d.V, vstride=d.vstride, cycles=d.cycles, n_spmm=d.steps,
                    converged=converged, history=history, scale=scale)

    def _eigsh_sigma(self, A, nev, sigma, b, m, keep, tol, max_cycles, B, lc, passes, inner, inner_tol,
                     inner_max_iter):
        """eigsh(sigma=...): see eigsh's docstring."""
        torch = _torch()
        if inner not in INNER_METHODS:
            raise LanczosError('eigsh: inner is "minres", "columns" or "block"')
        if not np.isfinite(sigma):
            raise LanczosError("eigsh: sigma must be finite")
        m, r = _restart_sizes("eigsh", "nev", nev, b, m, keep, A.n)
        n = A.n
        eps = float(np.finfo(np.float64 if A.val.dtype == torch.float64 else np.float32).eps)
        if inner_tol is None:
            inner_tol = max(INNER_TOL_FACTOR * tol, INNER_TOL_FLOOR_EPS * eps)
        inner_tol = float(inner_tol)
        if not inner_tol > 0.0:
            raise LanczosError("eigsh: inner_tol > 0")
        lo, hi = gershgorin(A)
        scale = max(abs(lo), abs(hi))
        info = InverseInfo()
        work = torch.empty(MINRES_WORK_BLOCKS * n * b, dtype=A.val.dtype, device=A.val.device)
        d = _Restart(self, A, n, b, m, r, lc, passes, A.val, inverse=(sigma, inner, inner_tol, inner_max_iter, info),
                     work=work)
        V, vstride, kw = d.V, d.vstride, d.kw
        U, X = work[:n * b].view(n, b), work[n * b:2 * n * b].view(n, b)  # (the solver's workspace is free between solves)
        C = torch.empty(r, b, b, **kw)
        dots = torch.empty(r, 2, b, dtype=torch.float64, device=A.val.device)
        rb = r * b

        def ran():
            if inner != "minres" and info.breakdown:
                raise LanczosError(f'eigsh: A - sigma I is not positive definite at sigma = {sigma} (inner="{inner}", '
                                   f'{info.breakdown} columns): use inner="minres"')

        def check():
            """Rayleigh-Ritz on A over the r kept blocks: (lambda ascending, true residual norms,
            the rb x rb rotation).  W and the panel are not touched."""
            H = np.empty((rb, rb))
            for i in range(r):
                self.spmm(A, V[i * vstride:i * vstride + n * b].view(n, b), U)
                self.panel_gram(V, vstride, r, U, C)  # C_j = Y_j^T A Y_i: block column i of H
                H[:, i * b:(i + 1) * b] = _f64(C).reshape(rb, b)
            lam, Cm = np.linalg.eigh(0.5 * (H + H.T))
            Sd = torch.from_numpy(_pack_chunks(Cm, r, b)).to(**kw)
            th = torch.from_numpy(lam).to(device=A.val.device)
            for c in range(r):
                self.panel_apply(0.0, 1.0, V, vstride, r, Sd[c], X)
                self.spmm_resid(A, X, th[c * b:(c + 1) * b], U, dots[c])
            res = np.sqrt(np.maximum(dots.cpu().numpy()[:, 0, :].reshape(rb), 0.0))
            return lam, res, Cm

        d.ran = ran  # (a broken-down inner solve leaves NaN blocks: name it before the rank test does)
        d.first(d.start_block(B))
        history = []
        while True:
            d.compress("magnitude")
            lam, res, Cm = check()
            sel = np.argsort(np.abs(lam - sigma), kind="stable")[:nev]
            history.append(float(res[sel].max()))
            converged = bool((res[sel] <= tol * scale).all())
            if converged or d.cycles >= max_cycles:
                break
            d.resume()
        Zx = _pack_chunks(Cm[:, sel], r, b)
        self.panel_compress(V, vstride, r, len(Zx), d._dev(Zx), n=n)
        return dict(theta=lam[sel], resid=res[sel], V=V, vstride=vstride, cycles=d.cycles, n_steps=d.steps,
                    n_spmm=int(info.n_spmm) + 2 * r * d.cycles, converged=converged, history=history, scale=scale,
                    sigma=sigma, inner=inner, inner_tol=inner_tol, inner_solves=int(info.solves),
                    inner_passes=int(info.passes), inner_not_met=int(info.not_met), inner_worst=float(info.worst),
                    inner_breakdown=int(info.breakdown))

    def svds(self, A: CsrDevice, k: int, b: int = 16, m: Optional[int] = None, keep: Optional[int] = None,
             tol: float = 1e-10, max_cycles: int = 100, B=None, lc: int = 0, passes: int = 2):
        """The k largest singular triplets of the sparse R x C operator A by thick-restart block
        Lanczos on G = P^T P, with P = A when C <= R and P = A^T otherwise, so that the Lanczos
        dimension is n = min(R, C).  A is transposed once (CsrDevice.transpose; returned as At),
        every operator line is Pt (P Q) (block_lanczos_reorth(normal=...)), and the loop is
        eigsh's with which = "largest": the same defaults and limits for m and keep, the same
        restart_coeffs, panel_compress, resume and restart_fill.  With theta the Ritz values of
        G, sigma_i = sqrt(max(theta_i, 0)), sigma_max = sqrt(max|theta| over all of T) and est_i
        the Ritz residual estimate on G, it stops when est_i <= tol * sigma_max * max(sigma_i,
        sqrt(eps) * sigma_max) for the k wanted pairs (eps: the epsilon of A's dtype) -- the
        estimate of ||A^T u_i - sigma_i v_i|| <= tol * ||A|| -- or after max_cycles cycles
        (converged = False, no exception).  Singular values below sqrt(eps) * sigma_max cannot be
        resolved through G (their squares drown in its rounding errors); the k smallest are
        out of scope for the same reason.

        The finish: one panel_compress leaves the k Ritz vectors x_i of G in the first ceil(k / b)
        blocks of the panel; per block, y = P x with every column scaled by 1 / ||column|| (zero
        columns stay zero) goes into a second panel of p-row blocks, and the measured residuals
        ||Pt y_i - sigma_i x_i|| come from one more SpMM and the dense kernels.  B (n, b): the
        start block, default uniform_B.  Returns a dict: s[k] descending; U, ustride, V, vstride
        (the left / right singular vectors as block-major panels of ceil(k / b) blocks of R / C
        rows, the last zero-padded); resid[k] measured; est[k]; cycles; n_spmm (every SpMM: two
        per Lanczos step, two per block of the finish); converged; history (the largest wanted
        est_i / (sigma_max * max(sigma_i, sqrt(eps) sigma_max)) of each cycle); At.

        Limits as eigsh's, on G: m * b <= n = min(R, C); a rank-deficient block (a deficient start
        block, an A of rank below m * b - b) raises LanczosError("... is rank deficient ...");
        a singular value of multiplicity above b is not guaranteed to come out complete."""
        torch = _torch()
        m, r = _restart_sizes("svds", "k", k, b, m, keep, min(A.n, A.n_cols))
        At = A.transpose(self)
        P, Pt = (A, At) if A.n_cols <= A.n else (At, A)
        n, p = P.n_cols, P.n
        work = torch.empty(p * b, dtype=A.val.dtype, device=A.val.device)
        d = _Restart(self, None, n, b, m, r, lc, passes, A.val, normal=(P, Pt, work))
        kw, W, xstride, ystride = d.kw, d.W, d.vstride, _panel_stride(p, b, A.val)
        eps = float(np.finfo(d.npdt).eps)
        d.first(d.start_block(B))
        history = []
        while True:
            theta, S, est, scale = d.ritz("largest")
            smax = float(np.sqrt(scale))
            theta, S, est = theta[:k], S[:, :k], est[:k]
            s = np.sqrt(np.maximum(theta, 0.0))
            ratio = est / (smax * np.maximum(s, np.sqrt(eps) * smax))
            history.append(float(ratio.max()))
            converged = bool(ratio.max() <= tol)
            if converged or d.cycles >= max_cycles:
                break
            d.compress("largest")
            d.resume()
        nch = d.pack(S, k)  # the wanted Ritz vectors of G, in place, into the first ceil(k / b) blocks
        X = d.V[:nch * xstride]
        # the other side: y = P x / ||P x||, and the measured residuals ||Pt y - sigma x||
        Y = torch.zeros(nch * ystride, **kw)
        Pw = work.view(p, b)
        Gm, Dm = torch.empty(b, b, **kw), torch.empty(b, b, **kw)
        resid = np.zeros(nch * b)
        sp = np.zeros(nch * b)
        sp[:k] = s
        for c in range(nch):
            Xc = X[c * xstride:c * xstride + n * b].view(n, b)
            Yc = Y[c * ystride:c * ystride + p * b].view(p, b)
            self.spmm(P, Xc, Pw)
            self.mm_tt(Pw, Gm)
            nrm = np.sqrt(np.maximum(np.diag(_f64(Gm)), 0.0))
            inv = np.divide(1.0, nrm, out=np.zeros_like(nrm), where=nrm > 0)
            Dm.copy_(torch.from_numpy(np.diag(inv)).to(**kw))
            self.mm_ts(0.0, 1.0, Pw, Dm, Yc)
            self.spmm(Pt, Yc, W)
            Dm.copy_(torch.from_numpy(np.diag(sp[c * b:(c + 1) * b])).to(**kw))
            self.mm_ts(1.0, -1.0, Xc, Dm, W)
            self.mm_tt(W, Gm)
            resid[c * b:(c + 1) * b] = np.sqrt(np.maximum(np.diag(_f64(Gm)), 0.0))
        U, ustride, Vv, vstride = (Y, ystride, X, xstride) if P is A else (X, xstride, Y, ystride)
        return dict(s=s, U=U, ustride=ustride, V=Vv, vstride=vstride, resid=resid[:k], est=est, cycles=d.cycles,
                    n_spmm=2 * (d.steps + nch), converged=converged, history=history, At=At)

    def _eigsh_cheb(self, d: _Restart, nev, which, tol, max_cycles, B, degree, cut):
        """eigsh(filter_degree=degree) on the driver eigsh set up (its docstring)."""
        torch = _torch()
        A, V, vstride, kw, n, b, m, r = d.A, d.V, d.vstride, d.kw, d.n, d.b, d.m, d.r
        nch = -(-nev // b)
        # 1. bounds: one unfiltered solve; its Ritz values place the filter
        d.first(B)
        theta, S, resid, scale = d.ritz(which)
        if resid[:nev].max() <= tol * scale:  # finished as the unfiltered eigsh finishes
            d.pack(S, nev)
            return dict(theta=theta[:nev], resid=resid[:nev], V=V, vstride=vstride, cycles=0, n_spmm=d.steps,
                        converged=True, history=[float(resid[:nev].max())], scale=scale, cols=np.arange(nev),
                        filter=None, n_steps=d.steps)
        # 2. the filter, fixed for the whole solve (the Lanczos relation across restarts needs
        # one operator).  The far end is Gershgorin's: a guaranteed enclosure, where a Lanczos
        # estimate that falls short would let p blow up.  theta_i >= lambda_i (Cauchy
        # interlacing), so the keep*b wanted eigenvalues lie outside the damped interval.
        g_lo, g_hi = gershgorin(A)
        asc = np.sort(theta)
        if which == "smallest":
            lo, hi, ref = (asc[r * b] if cut is None else float(cut)), g_hi, asc[0]
        else:
            lo, hi, ref = g_lo, (asc[-1 - r * b] if cut is None else float(cut)), asc[-1]
        if not lo < hi:
            raise LanczosError(f"eigsh: the damped interval [{lo}, {hi}] is empty (cut beyond the far end?)")
        if lo <= ref <= hi:
            raise LanczosError(f"eigsh: cut = {cut} leaves the outermost Ritz value {ref} inside the damped interval")
        filt = (degree, float(lo), float(hi), float(ref))
        work = torch.empty(2 * n * b, **kw)
        U = work[:n * b].view(n, b)  # the check's block (the filter's workspace is free between solves)
        Th, G = torch.empty(b, b, **kw), torch.empty(b, b, **kw)

        def check():
            """Rayleigh-Ritz on A within each of the first nch kept blocks Y_i: U = A Y_i, Theta_i =
            sym(Y_i^T U) = C Lambda C^T, R = U - Y_i Theta_i; the residual norms of the pairs
            (Lambda, Y_i C) are the column norms of R C, from R^T R.  W is not touched."""
            lam, res, Cs = [], [], []
            for i in range(nch):
                Yi = V[i * vstride:i * vstride + n * b].view(n, b)
                self.spmm(A, Yi, U)
                self.mm_tt2(U, Yi, Th)
                self.mm_ts(1.0, -1.0, Yi, Th, U)
                self.mm_tt(U, G)
                Thh, Gh = _f64(Th), _f64(G)
                lm, C = np.linalg.eigh(0.5 * (Thh + Thh.T))
                lam.append(lm)
                res.append(np.sqrt(np.maximum(np.einsum("ij,ik,kj->j", C, 0.5 * (Gh + Gh.T), C), 0.0)))
                Cs.append(C)
            return np.concatenate(lam), np.concatenate(res), Cs

        # 3. thick restart on p(A) from the same B: eigsh's loop, the largest end of T
        d.op = dict(filt=filt, work=work)
        d.first(B)
        history = []
        while True:
            d.compress("largest")
            # 4. the true residuals on A of the first nch kept blocks
            lam, res, Cs = check()
            # 5. the nev candidates at the wanted end
            sel = np.argsort(lam if which == "smallest" else -lam, kind="stable")[:nev]
            history.append(float(res[sel].max()))
            converged = bool(res[sel].max() <= tol * scale)
            if converged or d.cycles >= max_cycles:
                break
            d.resume()
        # block i <- Y_i C_i, in place: one compress over the nch blocks with a block-diagonal Z
        Zr = np.zeros((nch, nch, b, b))
        for i in range(nch):
            Zr[i, i] = Cs[i]
        self.panel_compress(V, vstride, nch, nch, torch.from_numpy(Zr).to(**kw), n=n)
        # SpMMs: the unfiltered solve's m, degree per filtered step, nch per check (one a cycle)
        return dict(theta=lam[sel], resid=res[sel], V=V, vstride=vstride, cycles=d.cycles,
                    n_spmm=m + (d.steps - m) * degree + nch * d.cycles, converged=converged, history=history,
                    scale=scale, cols=sel, filter=filt, n_steps=d.steps)

    def eigsh_interval(self, A: CsrDevice, a: float, b: float, /, block: int = 16, m: Optional[int] = None,
                       keep: Optional[int] = None, degree: Optional[int] = None, bounds=None, pad: float = 0.01,
                       tol: float = 1e-10, max_cycles: int = 100, B=None, lc: int = 0, passes: int = 2):
        """The eigenpairs of the symmetric operator A inside the window [a, b], anywhere in the
        spectrum, by thick-restart block Lanczos on p(A), p the Jackson-damped Chebyshev series
        of the window's indicator (cheb_window, cheb_series_apply): p is near 1 inside [a, b]
        and near 0 away from it, so the wanted pairs are the largest of p(A).

        Enclosure: bounds = (lo, hi), default gershgorin(A) (one copy of the CSR arrays to the
        host), each end moved out by pad x the width as spectral_moments does; [a, b] must lie
        inside it.  degree: default ceil(2 pi e / (b - a)) clipped to [16, 65536], e half the
        enclosure's width -- the degree that resolves the window, so the cost grows like
        n / (eigenvalues per window): the method serves windows that hold a fair share of the
        spectrum, or operators up to about 1e5 - 1e6 rows.  The coefficients are fixed for
        the whole solve.  m blocks in the panel, keep of them kept at a restart: keep <
        m <= PANEL_MAX_BLOCKS, keep <= PANEL_MAX_KEEP; default keep 4 (m - 1 if smaller), default
        m as eigsh's for nev = (keep - 1) * block.  The panel can hold at most keep * block - 1 pairs
        of the window.

        Every cycle: the restart of eigsh on p(A) at the largest end of T (first /
        compress / resume of the shared driver); after the compress, Rayleigh-Ritz on A over
        the whole kept subspace Y = [Y_0 .. Y_{keep-1}] -- p's values inside the window are
        nearly degenerate, so the kept Ritz vectors of p(A) mix across blocks: H = Y^T A Y from
        one SpMM and one panel_gram per kept block, eigh(H) on the host, the rotated vectors
        formed block by block (panel_apply into the series' free workspace) and their true
        residuals ||A x - lambda x|| measured with one more SpMM per block.  The panel itself
        is not rotated: the Lanczos relation of the restart stays intact.

        Stop test, with scale = max(|lo|, |hi|) of the widened enclosure (a bound of ||A||
        known before the first cycle): converged when every kept pair whose interval
        [lambda - res, lambda + res] meets [a, b] has res <= tol * scale and fewer than
        keep * block pairs lie in [a, b].  When all keep * block lie inside, the window may
        hold more than the panel keeps: it returns after that cycle with full = True,
        converged = False and no exception -- narrow the window or raise keep (eigcount sizes
        windows).  Otherwise it stops after max_cycles cycles (converged = False).

        Finish: one panel_compress packs the eigenvectors of the count pairs inside [a, b] into
        the first ceil(count / block) blocks of the panel, sorted by lambda ascending, the last
        zero-padded.  Returns a dict: theta[count] ascending, resid[count] (measured on A),
        count, V (the panel, flat), vstride, cycles, n_steps (Lanczos steps), n_spmm = degree *
        n_steps + 2 * keep * cycles (every SpMM: degree per step, 2 keep per cycle's check),
        converged, full, history (per cycle, the largest residual among the pairs that meet
        the window; 0 when none does), scale, filter = (degree, lo, hi).  Device memory that
        scales with n: the panel, W, B and 2 n block elements of workspace.  m * block <= n, and a
        rank-deficient block raises LanczosError, as in eigsh."""
        torch = _torch()
        a, b = float(a), float(b)
        if not a < b:
            raise LanczosError(f"eigsh_interval: the window [{a}, {b}] needs a < b")
        lo, hi = gershgorin(A) if bounds is None else (float(bounds[0]), float(bounds[1]))
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and pad >= 0):
            raise LanczosError(f"eigsh_interval: bounds ({lo}, {hi}) must be finite with lo < hi, pad >= 0")
        lo, hi = lo - pad * (hi - lo), hi + pad * (hi - lo)
        if not (lo <= a and b <= hi):
            raise LanczosError(f"eigsh_interval: the window [{a}, {b}] is not inside the enclosure [{lo}, {hi}]")
        if degree is None:
            degree = min(65536, max(16, int(np.ceil(np.pi * (hi - lo) / (b - a)))))
        if not 1 <= int(degree) <= 65536:
            raise LanczosError("eigsh_interval: 1 <= degree <= 65536")
        degree = int(degree)
        if keep is None:
            keep = 4 if m is None else max(1, min(4, m - 1))
        m, r = _restart_sizes("eigsh_interval", "(keep - 1) * block", max((keep - 1) * block, 1), block, m, keep,
                               A.n)
        n, bs = A.n, block
        scale = max(abs(lo), abs(hi))
        gamma = cheb_window(degree, lo, hi, a, b)
        work = torch.empty(2 * n * bs, dtype=A.val.dtype, device=A.val.device)
        d = _Restart(self, A, n, bs, m, r, lc, passes, A.val, series=(degree, lo, hi, gamma), work=work)
        V, vstride, kw = d.V, d.vstride, d.kw
        U, X = work[:n * bs].view(n, bs), work[n * bs:].view(n, bs)  # (the series' workspace is free between solves)
        C = torch.empty(r, bs, bs, **kw)
        G, Dm = torch.empty(bs, bs, **kw), torch.empty(bs, bs, **kw)
        rb = r * bs

        def check():
            """Rayleigh-Ritz on A over the r kept blocks: (lambda ascending, true residual norms,
            the rb x rb rotation).  W and the panel are not touched."""
            H = np.empty((rb, rb))
            for i in range(r):
                self.spmm(A, V[i * vstride:i * vstride + n * bs].view(n, bs), U)
                self.panel_gram(V, vstride, r, U, C)  # C_j = Y_j^T A Y_i: block column i of H
                H[:, i * bs:(i + 1) * bs] = _f64(C).reshape(rb, bs)
            lam, Cm = np.linalg.eigh(0.5 * (H + H.T))
            Sd = torch.from_numpy(_pack_chunks(Cm, r, bs)).to(**kw)
            res = np.empty(rb)
            for c in range(r):
                self.panel_apply(0.0, 1.0, V, vstride, r, Sd[c], X)
                self.spmm(A, X, U)
                Dm.copy_(torch.from_numpy(np.diag(lam[c * bs:(c + 1) * bs])).to(**kw))
                self.mm_ts(1.0, -1.0, X, Dm, U)
                self.mm_tt(U, G)
                res[c * bs:(c + 1) * bs] = np.sqrt(np.maximum(np.diag(_f64(G)), 0.0))
            return lam, res, Cm

        d.first(d.start_block(B))
        history = []
        while True:
            d.compress("largest")
            lam, res, Cm = check()
            meets = (lam + res >= a) & (lam - res <= b)
            inside = (lam >= a) & (lam <= b)
            full = bool(inside.sum() == rb)
            history.append(float(res[meets].max()) if meets.any() else 0.0)
            converged = bool(not full and (res[meets] <= tol * scale).all())
            if converged or full or d.cycles >= max_cycles:
                break
            d.resume()
        sel = np.flatnonzero(inside)  # (eigh: lambda ascending)
        if sel.size:
            Zx = _pack_chunks(Cm[:, sel], r, bs)
            self.panel_compress(V, vstride, r, len(Zx), d._dev(Zx), n=n)
        return dict(theta=lam[sel], resid=res[sel], count=int(sel.size), V=V, vstride=vstride, cycles=d.cycles,
                    n_steps=d.steps, n_spmm=degree * d.steps + 2 * r * d.cycles, converged=converged, full=full,
                    history=history, scale=scale, filter=(degree, lo, hi))

    def set_final_state(self, on: bool) -> None:
        """True (default): block_lanczos_blas leaves Q0 = Q1 = Q_{m-1} and W = the
        last residual, as the reference does; False: they are scratch on return."""
        _check(self.L.lz_set_final_state(self.ptr, 1 if on else 0), "lz_set_final_state")

    def vector_lanczos(self, A: CsrDevice, bvec, m: int, lc: int, q, alpha, beta, q0, q1, w):
        """vector_lanczos (methods/vector_lanczos.hpp:8-67); alpha/beta are device tensors.
        fp64 or fp32: every vector must have A's element type."""
        n = bvec.shape[0]
        for t in (bvec, q, alpha, beta, q0, q1, w):
            if t.element_size() != (8 if A.dtype == LZ_F64 else 4):
                raise ValueError("vector_lanczos: every vector must have A's element type")
        _check(self.L.lz_vector_lanczos(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype,
                                        m, lc, _ptr(bvec), _ptr(q), _ptr(alpha), _ptr(beta), _ptr(q0),
                                        _ptr(q1), _ptr(w)), "lz_vector_lanczos")

    def ftdt_block(self, A: CsrDevice, U0, steps: int, T_end: float, lc: int, U, D, out):
        n, b = U0.shape
        _check(self.L.lz_fdtd_block(self.ptr, n, A.nnz, _ptr(A.row_ptr), _ptr(A.col), _ptr(A.val), A.dtype, b,
                                    _ptr(U0), steps, T_end, lc, _ptr(U), _ptr(D), _ptr(out)), "lz_fdtd_block")
        return out

    # --- hipEvent timing of kernel classes ------------------------------
    PROF_SPMM_PASS, PROF_UPDATE_PASS, PROF_SMALL, PROF_GRAM, PROF_TSMM, PROF_SPMM = range(6)

    def device_error(self) -> int:
        """Synchronise and return (then clear) the device error word (0 = ok)."""
        c = _c_int()
        _check(self.L.lz_device_error(self._h, ctypes.byref(c)), "lz_device_error")
        return c.value

    def debug_set_device_error(self, code: int):
        """Store `code` into the device error word (test support)."""
        _check(self.L.lz_debug_set_device_error(self.ptr, code), "lz_debug_set_device_error")

    def debug_fail_next_setup(self, code: int = 5):
        """The next distributed solve on this handle fails its set-up with `code`
        on this rank (test support: its peers must return, not wait)."""
        _check(self.L.lz_debug_fail_next_setup(self._h, code), "lz_debug_fail_next_setup")

    def debug_poison_lds(self, pattern: int = 0xFFFFFFFF):
        """Fill every CU's LDS with `pattern` (test support: stale-LDS reads show as NaN)."""
        _check(self.L.lz_debug_poison_lds(self._h, pattern), "lz_debug_poison_lds")

    def prof_enable(self, on: bool = True, classes=None):
        """Record kernel-class timings (all classes, or only `classes`)."""
        if classes is None:
            _check(self.L.lz_prof_enable(self._h, int(on)), "lz_prof_enable")
        else:
            mask = 0
            for c in classes:
                mask |= 1 << int(c)
            _check(self.L.lz_prof_enable_mask(self._h, mask if on else 0), "lz_prof_enable_mask")

    def prof_read(self, cls: int):
        """(total ms, launches) of a kernel class since prof_enable."""
        ms, cnt = _c_dbl(), _c_int()
        _check(self.L.lz_prof_read(self._h, cls, ctypes.byref(ms), ctypes.byref(cnt)), "lz_prof_read")
        return ms.value, cnt.value

    # --- multi-GPU ------------------------------------------------------
    def comm_init(self, nranks: int, rank: int, uid: bytes):
        buf = ctypes.create_string_buffer(uid, 128)
        _check(self.L.lz_comm_init(self._h, nranks, rank, buf), "lz_comm_init")

    def comm_init_local(self, group: "LocalGroup", rank: int):
        """Attach this handle as virtual rank `rank` of an in-process group (one device)."""
        _check(self.L.lz_comm_init_local(self.ptr, group.ptr, rank), "lz_comm_init_local")
        group._keep.append(self)

    def last_wf(self):
        """(wavefront step, pass-2-first overlap) flags of the last distributed solve."""
        v = (_c_int * 2)()
        _check(self.L.lz_debug_last_wf(self._h, v), "lz_debug_last_wf")
        return bool(v[0]), bool(v[1])

    def last_kernel(self):
        """(SpMM-family id, dense-family id) of the handle's last launches (LZ_K_*; 0: none yet)."""
        v = (_c_int * 2)()
        _check(self.L.lz_debug_last_kernel(self._h, v), "lz_debug_last_kernel")
        return int(v[0]), int(v[1])

    def wf_plan(self, A, nx=None, xoff=0):
        """The wavefront step's plan of device operator A (test hook): (info dict,
        deps (T, 2) int32 tensor, col16 (nnz,) int16 tensor)."""
        import torch
        T_max = A.n // 16 + 2
        deps = torch.zeros(T_max * 2, dtype=torch.int32, device=A.row_ptr.device)
        c16 = torch.zeros(max(A.nnz, 1), dtype=torch.int16, device=A.row_ptr.device)
        info = (_c_int * 8)()
        _check(self.L.lz_debug_wf_plan(self.ptr, A.n, A.nnz, A.row_ptr.data_ptr(), A.col.data_ptr(),
                                       A.n if nx is None else nx, xoff, deps.data_ptr(), c16.data_ptr(), info),
               "lz_debug_wf_plan")
        T = int(info[2])
        d = {"ok": bool(info[0]), "col16": bool(info[1]), "T": T, "tr": int(info[3]),
             "spans": [int(info[4 + i]) for i in range(4)]}
        return d, deps[: 2 * T].view(T, 2), c16[: A.nnz]

    def last_split(self):
        """(i0, i1) of the last distributed solve's interior rows (pass 1 beside the
        exchange), or None when it ran unsplit."""
        v = (_c_i64 * 2)()
        _check(self.L.lz_debug_last_split(self._h, v), "lz_debug_last_split")
        return None if v[0] < 0 else (int(v[0]), int(v[1]))

    def comm_abort(self):
        _check(self.L.lz_comm_abort(self._h), "lz_comm_abort")

    def comm_destroy(self):
        _check(self.L.lz_comm_destroy(self._h), "lz_comm_destroy")

    def block_lanczos_dist(self, A_local: CsrDevice, n_pad: int, n_global: int, B_local, m: int,
                           lc_local: int, lc_rank: int, q, alpha, beta, Q0, W, X_full):
        n_local, b = A_local.n, B_local.shape[1]
        _check(self.L.lz_block_lanczos_dist(self.ptr, n_local, n_pad, n_global, A_local.nnz,
                                            _ptr(A_local.row_ptr), _ptr(A_local.col), _ptr(A_local.val),
                                            A_local.dtype, b, m, lc_local, lc_rank, _ptr(B_local), _ptr(q),
                                            _ptr(alpha), _ptr(beta), _ptr(Q0), None, _ptr(W), _ptr(X_full)),
               "lz_block_lanczos_dist")


    def halo_init(self, row0: int, n_local: int, recv_counts: np.ndarray, halo_rows: np.ndarray):
        rc = np.ascontiguousarray(recv_counts, np.int64)
        hr = np.ascontiguousarray(halo_rows, np.int32)
        _check(self.L.lz_halo_init(self.ptr, row0, n_local, _p(rc), _p(hr) if hr.size else None),
               "lz_halo_init")

    def halo_sizes(self):
        nh, ns = _c_i64(), _c_i64()
        _check(self.L.lz_halo_sizes(self.ptr, ctypes.byref(nh), ctypes.byref(ns)), "lz_halo_sizes")
        return nh.value, ns.value

    def halo_exchange(self, X):
        _check(self.L.lz_halo_exchange(self.ptr, _dt(X), X.shape[1], _ptr(X)), "lz_halo_exchange")

    def block_lanczos_halo(self, A_local: CsrDevice, B_local, m: int, lc_local: int, lc_rank: int,
                           q, alpha, beta, X0, X1):
        """Distributed block Lanczos over the halo plan (A_local.col in the compact numbering)."""
        n_local, b = A_local.n, B_local.shape[1]
        _check(self.L.lz_block_lanczos_halo(self.ptr, n_local, A_local.nnz, _ptr(A_local.row_ptr),
                                            _ptr(A_local.col), _ptr(A_local.val), A_local.dtype, b, m,
                                            lc_local, lc_rank, _ptr(B_local), _ptr(q), _ptr(alpha),
                                            _ptr(beta), _ptr(X0), _ptr(X1)),
               "lz_block_lanczos_halo")


class LocalGroup:
    """N virtual ranks on one device in this process (lz_local_group_create):
    every rank's Handle attaches with comm_init_local and then runs the same
    distributed entry points an RCCL rank runs, from its own thread."""

    def __init__(self, nranks: int, device: int = 0):
        L = hip_lib()
        g = _c_vp()
        _check(L.lz_local_group_create(device, nranks, ctypes.byref(g)), "lz_local_group_create")
        self.ptr, self.nranks, self.device, self.L = g, nranks, device, L
        self._keep = []

    def abort(self):
        if self.ptr:
            self.L.lz_local_group_abort(self.ptr)

    def close(self):
        if self.ptr:
            self.L.lz_local_group_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_virtual_ranks(nranks: int, fn, device: int = 0, timeout: float = 600.0):
    """Run fn(rank, handle) for ranks 0..nranks-1, each in its own thread with its
    own torch stream and its own lz Handle attached to one LocalGroup.  Inputs
    made before the call are synchronised first; returns the list of results.
    A rank that raises aborts the group, so no other rank waits for it."""
    import threading
    torch = _torch()
    torch.cuda.synchronize(device)
    group = LocalGroup(nranks, device)
    handles = [Handle(device) for _ in range(nranks)]
    # the ranks' streams are made here and outlive every handle (closed below
    # after a device synchronise), so no handle ever refers to a stream whose
    # Python object a finished thread dropped
    streams = [torch.cuda.Stream(device) for _ in range(nranks)]
    out, errs = [None] * nranks, [None] * nranks

    def body(r):
        try:
            with torch.cuda.device(device), torch.cuda.stream(streams[r]):
                handles[r].comm_init_local(group, r)
                out[r] = fn(r, handles[r])
                torch.cuda.current_stream(device).synchronize()
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs[r] = e
            group.abort()

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(nranks)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout)
        if any(t.is_alive() for t in threads):
            group.abort()
            for t in threads:
                t.join(30)
        if any(t.is_alive() for t in threads):  # never free what a live thread may still use
            raise LanczosError("virtual ranks did not finish")
    finally:
        if not any(t.is_alive() for t in threads):
            torch.cuda.synchronize(device)
            for h in handles:
                h.close()
            group.close()
            group._keep.clear()
            del streams[:]
    for r, e in enumerate(errs):
        if e is not None:
            raise LanczosError(f"virtual rank {r}: {e}") from e
    return out


def comm_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(hip_lib().lz_comm_unique_id(buf), "lz_comm_unique_id")
    return buf.raw


def run_block_lanczos(h: Handle, A: CsrDevice, B, m: int, lc: int, fused: bool = True):
    """Allocate the reference's workspaces and run block_lanczos_blas; returns device
    tensors (q, alpha, beta)."""
    torch = _torch()
    n, b = B.shape
    kw = dict(dtype=B.dtype, device=B.device)
    q = torch.zeros(m * b, **kw)
    alpha = torch.zeros(m, b, b, **kw)
    beta = torch.zeros(m + 1, b, b, **kw)
    Q0, Q1, W = (torch.empty(n, b, **kw) for _ in range(3))
    h.block_lanczos_blas(A, B, m, lc, q, alpha, beta, Q0, Q1, W, fused=fused)
    return q, alpha, beta
