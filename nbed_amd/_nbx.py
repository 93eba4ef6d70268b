"""ctypes binding of libnbx (include/nbx.h) -- the thin FFI layer.

Only plain pointers and sizes cross this boundary.  The product path fails
loudly (``NbxUnavailableError``) when the shared library is missing; there is no
CPU fallback anywhere in ``nbed_amd``.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p
from pathlib import Path

LIB_NAME = "libnbx.so"
LIB_PATH = Path(__file__).resolve().parent / LIB_NAME

NBX_VERSION = 3  # the include/nbx.h this table mirrors (buffer sizes behind the entry points: see the header)
NBX_OK = 0
NBX_E_INVALID = -1
NBX_E_HIP = -2
NBX_E_NOMEM = -3
NBX_E_NOCONV = -4
NBX_E_UNSUPPORTED = -5
NBX_E_INTERNAL = -6
LOC_PM, LOC_BOYS = 0, 1  # nbx_loc_worksize kinds (NBX_LOC_PM, NBX_LOC_BOYS)

HUZ_JK_PACKED, HUZ_JK_SYM = 0, 1
XC_CODES = {"slater": 0, "lda": 1, "lda,vwn_rpa": 1, "lda,vwn": 2, "lda,vwn5": 2, "svwn": 2, "b3lyp": 3, "lda,pw_mod": 4,
            "pbe": 5, "pbe,pbe": 5, "pbeh": 6, "pbe1pbe": 6, "blyp": 7, "b3lyp5": 8}
XC_RS_CODES = {"cam-b3lyp": 16, "camb3lyp": 16, "lc-blyp": 17}  # nbx_xc_functional_rs (NBX_XC_CAM_B3LYP, NBX_XC_LC_BLYP)
XC_MGGA_CODES = {"tpss": 32, "tpssh": 33}  # nbx_xc_functional_mgga (NBX_XC_TPSS, NBX_XC_TPSSH)

PROF_JK_DENSE, PROF_AO2MO_Q1, PROF_AO2MO, PROF_EIGH, PROF_SVD, PROF_GEMM = range(6)
PROF_ERI = 7  # the class launches of nbx_eri_device (nbx_eri_class_ms)
ERI_CLASSES = 25  # (la + lb, lc + ld), index 5 l_ab + l_cd
# nbx_gemm_route answers (NBX_GEMM_KERNEL_*)
GEMM_KERNEL_NONE, GEMM_KERNEL_SMALL, GEMM_KERNEL_T32, GEMM_KERNEL_T64, GEMM_KERNEL_T128, GEMM_KERNEL_TN_DMA = range(6)
# nbx_jk_packed_route answers (NBX_JK_KERNEL_*)
JK_KERNEL_NONE, JK_KERNEL_S4, JK_KERNEL_M4, JK_KERNEL_M8, JK_KERNEL_MX, JK_KERNEL_MX_HI = range(6)
# nbx_cycle_scalars_route / nbx_diis_route / nbx_vo_sumsq_route answers (NBX_CYCLE_SCALARS_*, NBX_DIIS_*, NBX_VO_SUMSQ_*)
CYCLE_SCALARS_REFUSED, CYCLE_SCALARS_T32, CYCLE_SCALARS_T16, CYCLE_SCALARS_T16_DENS = range(4)
DIIS_REFUSED, DIIS_FUSED, DIIS_GENERAL = range(3)
VO_SUMSQ_REFUSED, VO_SUMSQ_ONE_WG, VO_SUMSQ_32_WG = range(3)


class NbxError(RuntimeError):
    """A libnbx entry point returned an error code."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libnbx error {code}: {message}")
        self.code = code


class NbxUnavailableError(RuntimeError):
    """libnbx.so is not built or no MI355X is visible: the HIP path cannot run."""


class HuzState(ctypes.Structure):
    """``nbx_huz_state`` of include/nbx.h: the device pointers one SCF keeps for ``nbx_huz_cycle``."""

    _fields_ = [
        ("nao", c_int64), ("nocc_a", c_int64), ("nocc_b", c_int64),
        ("d_packed", c_void_p), ("d_hv", c_void_p), ("d_ds", c_void_p), ("d_sb", c_void_p), ("d_x", c_void_p),
        ("d_dts", c_void_p), ("d_jk", c_void_p), ("d_fock", c_void_p), ("d_vhf", c_void_p), ("d_fock2", c_void_p),
        ("d_tmp", c_void_p), ("d_fo", c_void_p),
        ("d_jk_work", c_void_p), ("jk_work_bytes", c_size_t),
        ("d_eig_work", c_void_p), ("eig_work_bytes", c_size_t),
        ("d_geig_work", c_void_p), ("geig_work_bytes", c_size_t),
        ("diis_space", c_int64), ("d_diis_xs", c_void_p), ("d_diis_es", c_void_p), ("d_diis_h", c_void_p),
        ("d_diis_coef", c_void_p), ("d_diis_xprev", c_void_p),
        ("jk_kind", c_int64), ("jk_p0", c_int64), ("jk_p1", c_int64), ("d_eri", c_void_p),
        ("d_scal_partial", c_void_p),
    ]


HUZ_PARTIAL_DOUBLES = 4096  # NBX_HUZ_PARTIAL_DOUBLES: the doubles behind HuzState.d_scal_partial


class ScalarsCourier(ctypes.Structure):
    """``nbx_scalars_courier`` of include/nbx.h: what is left to do for a cycle whose scalars were deferred
    (``nbx_huz_cycle_carry`` fills it; the next call, or ``nbx_huz_scalars_flush``, is handed it)."""

    _fields_ = [
        ("d_partial", c_void_p), ("nblocks", c_int32), ("nthreads", c_int32), ("d_status", c_void_p),
        ("nstatus", c_int32), ("reserved", c_int32), ("h_out", c_void_p),
    ]


# name -> (restype, argtypes); mirrors include/nbx.h one to one
_P = c_void_p
SIGNATURES = {
    "nbx_version": (c_int, []),
    "nbx_last_error": (c_char_p, []),
    "nbx_device_count": (c_int, [POINTER(c_int)]),
    "nbx_ctx_create": (c_int, [c_int, _P, c_int, POINTER(_P)]),
    "nbx_ctx_destroy": (c_int, [_P]),
    "nbx_ctx_set_stream": (c_int, [_P, _P]),
    "nbx_sync": (c_int, [_P]),
    "nbx_malloc": (c_int, [_P, c_size_t, POINTER(_P)]),
    "nbx_free": (c_int, [_P, _P]),
    "nbx_memcpy_h2d": (c_int, [_P, _P, _P, c_size_t]),
    "nbx_memcpy_d2h": (c_int, [_P, _P, _P, c_size_t]),
    "nbx_gather_to_host": (c_int, [_P, c_int64, _P, _P, _P, c_int]),
    "nbx_jk_df_worksize": (c_size_t, [c_int64, c_int64, c_int64]),
    "nbx_jk_df": (c_int, [_P, c_int64, c_int64, _P, c_int64, _P, POINTER(c_int64), _P, _P, c_size_t]),
    "nbx_df_synth": (c_int, [_P, c_int64, c_int64, c_int64, c_uint64, c_double, _P]),
    "nbx_memcpy_d2d": (c_int, [_P, _P, _P, c_size_t]),
    "nbx_memset": (c_int, [_P, _P, c_int, c_size_t]),
    "nbx_profile_enable": (c_int, [_P, c_int]),
    "nbx_profile_sample": (c_int, [_P, c_int]),
    "nbx_debug_fill_lds": (c_int, [_P, c_double]),
    "nbx_profile_read": (c_int, [_P, c_int, POINTER(c_double), POINTER(c_int64)]),
    "nbx_profile_reset": (c_int, [_P]),
    "nbx_synth_eri": (c_int, [_P, c_int64, c_int64, c_int64, c_uint64, _P]),
    "nbx_jk_dense_worksize": (c_size_t, [c_int64, c_int64, c_int64]),
    "nbx_jk_dense": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_size_t]),
    "nbx_jk_dense_sym_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_jk_packed_supported": (c_int, [c_int64]),
    "nbx_jk_packed_fold": (c_int, [c_int64]),
    "nbx_jk_packed_route": (c_int, [c_int64, POINTER(c_int), POINTER(c_int)]),
    "nbx_eri_packed_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "nbx_eri_pack": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P]),
    "nbx_jk_packed_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_huzinaga_fused": (c_int, [_P, c_int64, c_int64, _P, _P, c_double, _P, _P]),
    "nbx_jk_packed_fock": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nbx_jk_dts_bytes": (c_size_t, [c_int64]),
    "nbx_jk_dts_init": (c_int, [_P, c_int64, _P]),
    "nbx_jk_packed": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_size_t]),
    "nbx_jk_dense_sym": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, c_size_t]),
    "nbx_jk_synth_sym_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_jk_synth_sym": (c_int, [_P, c_int64, c_int64, c_int64, c_uint64, _P, c_int64, _P, _P, c_size_t]),
    "nbx_jk_synth": (c_int, [_P, c_int64, c_int64, c_int64, c_uint64, _P, c_int64, _P, _P, c_size_t]),
    "nbx_gemm": (c_int, [_P, c_char, c_char, c_int64, c_int64, c_int64, c_double, _P, c_int64, c_int64,
                         _P, c_int64, c_int64, c_double, _P, c_int64, c_int64, c_int64]),
    "nbx_gemm_route": (c_int, [c_char, c_char, c_int64, c_int64, c_int64, c_int64, c_int, c_int]),
    "nbx_fock_uhf": (c_int, [_P, c_int64, _P, c_int, _P, _P, _P, _P]),
    "nbx_huzinaga_sym": (c_int, [_P, c_int64, c_int64, _P, c_double, _P, _P]),
    "nbx_trace_prod": (c_int, [_P, c_int64, c_int64, _P, _P, POINTER(c_double)]),
    "nbx_huz_cycle_scalars": (c_int, [_P, c_int64, _P, c_int, _P, _P, _P, _P, _P, POINTER(c_double)]),
    "nbx_huz_cycle_scalars_dev": (c_int, [_P, c_int64, _P, c_int, _P, _P, _P, _P, _P, _P, _P, c_int64]),
    "nbx_huz_cycle_scalars_dts": (c_int, [_P, c_int64, _P, c_int, _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
    "nbx_diis_coef_doubles": (c_size_t, [c_int64]),
    "nbx_diis_update": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P]),
    "nbx_diis_update_err": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "nbx_vo_sumsq": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P]),
    "nbx_axpby": (c_int, [_P, c_int64, c_double, _P, c_double, _P]),
    "nbx_lincomb": (c_int, [_P, c_int64, c_int64, POINTER(c_double), _P, c_int64, _P]),
    "nbx_dots": (c_int, [_P, c_int64, c_int64, _P, _P, c_int64, POINTER(c_double)]),
    "nbx_transpose": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P]),
    "nbx_scale_cols": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P]),
    "nbx_cycle_scalars_route": (c_int, [c_int64, c_int64, c_int64]),
    "nbx_diis_route": (c_int, [c_int64, c_int64]),
    "nbx_vo_sumsq_route": (c_int, [c_int64, c_int64, c_int64]),
    "nbx_eigh_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_eigh": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, c_size_t]),
    "nbx_eigh_warm": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, c_size_t]),
    "nbx_geig_refine_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_geig_refine": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, c_size_t, c_int]),
    "nbx_eigh_warm_ex": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, c_size_t, c_int]),
    "nbx_eigh_status_offset": (c_size_t, [c_int64, c_int64]),
    "nbx_eigh_approx_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_eigh_approx": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "nbx_eigh_status": (c_int, [_P, c_int64, c_int64, _P, POINTER(c_int)]),
    "nbx_sym_pow_worksize": (c_size_t, [c_int64]),
    "nbx_sym_pow": (c_int, [_P, c_int64, _P, c_double, _P, _P, c_size_t]),
    "nbx_sym_pow_ns_worksize": (c_size_t, [c_int64]),
    "nbx_sym_pow_ns": (c_int, [_P, c_int64, _P, c_double, c_double, _P, _P, c_size_t, c_int, c_int, POINTER(c_int)]),
    "nbx_svd_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_svd_right": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, c_size_t]),
    "nbx_svd_status": (c_int, [_P, c_int64, c_int64, _P, POINTER(c_int)]),
    "nbx_loc_worksize": (c_size_t, [c_int, c_int, c_int64, c_int64, c_int64]),
    "nbx_loc_pm": (c_int, [_P, c_int, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_int, c_double, _P, c_size_t]),
    "nbx_loc_boys": (c_int, [_P, c_int, c_int64, _P, _P, c_int, c_double, _P, c_size_t]),
    "nbx_loc_status": (c_int, [_P, c_int, _P, POINTER(c_int), POINTER(c_double)]),
    "nbx_ao2mo_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo": (c_int, [_P, c_int64, _P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P,
                          c_int64, _P, _P, c_size_t]),
    "nbx_ao2mo_pair_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo_pair": (c_int, [_P, c_int64, _P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64,
                               _P, _P, c_int64, _P, c_int64, _P, _P, c_size_t]),
    "nbx_ao2mo_pair_sym_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo_pair_sym": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64,
                                   _P, _P, c_size_t]),
    "nbx_eri_rs_bytes": (c_size_t, [c_int64]),
    "nbx_eri_pack_rs": (c_int, [_P, c_int64, _P, _P]),
    "nbx_ao2mo_pair_sym_rs_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo_pair_sym_rs": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P,
                                      c_int64, _P, _P, c_size_t]),
    "nbx_ao2mo_synth_pair_worksize": (c_size_t, [c_int64] * 7),
    "nbx_ao2mo_synth_pair": (c_int, [_P, c_int64, c_uint64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64,
                                     _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P, c_size_t]),
    "nbx_ao2mo_synth_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo_synth": (c_int, [_P, c_int64, c_uint64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P,
                                c_int64, _P, _P, c_size_t]),
    "nbx_chem_to_phys": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, _P]),
    "nbx_spinorb_scatter_h1": (c_int, [_P, c_int64, _P, c_double, _P]),
    "nbx_spinorb_scatter_range": (c_int, [_P, c_int64, _P, c_double, c_double, c_int64, c_int64, _P]),
    "nbx_spinorb_scatter": (c_int, [_P, c_int64, _P, _P, c_double, c_double, _P, _P]),
    "nbx_threshold_scale": (c_int, [_P, c_int64, c_double, c_double, _P]),
    "nbx_becke_share": (c_int, [_P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P]),
    "nbx_eval_ao": (c_int, [_P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int64, _P, _P]),
    "nbx_xc_rho": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "nbx_xc_functional_worksize": (c_size_t, [c_int64]),
    "nbx_xc_functional": (c_int, [_P, c_int, c_int64, _P, _P, _P, c_double, _P, _P, _P, _P, c_size_t]),
    "nbx_xc_functional_rs": (c_int, [_P, c_int, c_double, c_int64, _P, _P, _P, c_double, _P, _P, _P, _P, c_size_t]),
    "nbx_xc_vmat_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_xc_rho_tau": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P]),
    "nbx_xc_functional_mgga": (c_int, [_P, c_int, c_int64, _P, _P, _P, _P, c_double, _P, _P, _P, _P, _P, c_size_t]),
    "nbx_xc_vmat_tau_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_xc_vmat_tau": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, c_size_t]),
    "nbx_xc_vmat": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, c_size_t]),
    "nbx_purify_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_purify": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, _P, _P, c_size_t, c_int, _P]),
    "nbx_host_1e": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, c_int, _P, _P, _P]),
    "nbx_host_eri": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_int, _P]),
    "nbx_host_eri_erf": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_double, c_int, _P]),
    "nbx_host_dipole": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "nbx_eri_device": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, _P]),
    "nbx_eri_device_erf": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_double, _P]),
    "nbx_eri_class_ms": (c_int, [_P, POINTER(c_double)]),
    "nbx_eri_plan": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_double, POINTER(c_int64), POINTER(c_int), POINTER(c_int),
                             POINTER(c_int64)]),
    "nbx_eri_diagonal": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, _P]),
    "nbx_eri_columns": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_int, _P, _P, _P]),
    "nbx_eri_cholesky": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_double, c_int64, _P, POINTER(c_int64),
                                 POINTER(c_double)]),
    "nbx_eri_cholesky_steps": (c_int, [POINTER(c_int64), POINTER(c_int64)]),
    "nbx_host_mm_potential": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, c_int, _P]),
    "nbx_mm_potential": (c_int, [_P, c_int, _P, _P, _P, _P, _P, _P, _P, c_double, c_int, _P, _P, _P, _P]),
    "nbx_ao2mo_factor_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "nbx_ao2mo_factor": (c_int, [_P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int64, _P, _P, _P, _P,
                                 c_size_t]),
    "nbx_ao2mo_factor_half": (c_int, [_P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int64, _P]),
    "nbx_ao2mo_factor_expand": (c_int, [_P, c_int64, _P, _P]),
    "nbx_huz_cycle": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                              c_int, _P, _P]),
    "nbx_huz_cycle_carry": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                    c_int, _P, _P, POINTER(ScalarsCourier), c_int, POINTER(ScalarsCourier)]),
    "nbx_huz_scalars_flush": (c_int, [_P, POINTER(ScalarsCourier)]),
    "nbx_huz_cycle_jk": (c_int, [_P, POINTER(HuzState), _P]),
    "nbx_mu_cycle": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                             c_int, _P, _P]),
    "nbx_mu_cycle_solve": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                   _P]),
    "nbx_mu_cycle_fock": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, c_int, _P, _P]),
    "nbx_mu_cycle_fock_post": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, c_int, _P, _P]),
    "nbx_huz_cycle_post": (c_int, [_P, POINTER(HuzState), _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                   _P, _P]),
    "nbx_ccsd_gather": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int, c_int, _P]),
    "nbx_ccsd_fock": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P]),
    "nbx_permute4": (c_int, [_P, POINTER(c_int64), POINTER(c_int), c_double, _P, c_double, _P]),
    "nbx_pair_pack": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P]),
    "nbx_pair_unpack": (c_int, [_P, c_int64, c_int64, c_int64, c_double, _P, c_double, _P]),
    "nbx_ccsd_tau": (c_int, [_P, c_int64, c_int64, _P, _P, c_double, c_double, c_double, c_int, _P]),
    "nbx_ccsd_update": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "nbx_ccsd_lambda_outer": (c_int, [_P, c_int64, c_int64, c_double, _P, _P, c_int, _P]),
    "nbx_ccsd_rdm1": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nbx_ccsd_triples_worksize": (c_size_t, [c_int64, c_int64]),
    "nbx_ccsd_triples_tile": (c_int, []),
    "nbx_ccsd_triples_energy": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "nbx_mp2_pairs_worksize": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int]),
    "nbx_mp2_pairs_tile": (c_int, []),
    "nbx_mp2_pairs": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, c_int, _P, _P, c_size_t, _P]),
    "nbx_fci_gmat": (c_int, [_P, c_int64, _P, _P, _P]),
    "nbx_fci_gather": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P]),
    "nbx_fci_scatter": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_double, _P, c_int, _P]),
    "nbx_fci_diag": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_double, _P]),
    "nbx_fci_precond": (c_int, [_P, c_int64, c_double, c_double, _P, _P, _P]),
    "nbx_fci_rdm_finish": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P]),
    "nbx_fci_rdm1": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P]),
}

_lib = None


def load_library(path: os.PathLike | None = None) -> ctypes.CDLL:
    """dlopen libnbx.so and attach the prototypes of include/nbx.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("NBX_LIB"):  # an alternative build of the library (A/B measurements)
        path = os.environ["NBX_LIB"]
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise NbxUnavailableError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); nbed_amd has no CPU fallback."
        )
    try:
        # torch ships its own libamdhip64.so (same SONAME as /opt/rocm's): load torch first so
        # that libnbx binds to the one HIP runtime already in the process.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch-less FFI users get the system runtime
        pass
    lib = ctypes.CDLL(str(p), mode=ctypes.RTLD_GLOBAL)
    lib.nbx_version.restype = c_int
    if lib.nbx_version() != NBX_VERSION:
        raise NbxUnavailableError(
            f"{p} is ABI version {lib.nbx_version()}, this package binds version {NBX_VERSION} (include/nbx.h): "
            "rebuild it (`make -C nbed_amd/csrc`) -- buffer sizes behind several entry points differ between versions"
        )
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _lib = lib
    return lib


def check(lib: ctypes.CDLL, rc: int) -> None:
    if rc != NBX_OK:
        msg = lib.nbx_last_error()
        raise NbxError(rc, msg.decode() if msg else "")
