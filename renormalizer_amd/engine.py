"""ctypes binding of libmpsengine.so (include/mpsengine.h) and device-resident tensors.

This is the only place where Python touches the GPU: no PyTorch, no CuPy.  If the
HIP library is missing or no GPU is visible the engine refuses to start - there is
deliberately no CPU fallback (the NumPy restatement lives in ``oracle/`` and is
test infrastructure only).
"""
import collections
import ctypes as C
import math
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RENO_MPSENGINE overrides the in-tree library; there is still no CPU fallback
LIB_PATH = os.environ.get("RENO_MPSENGINE") or os.path.join(_HERE, "csrc", "libmpsengine.so")

F64, C128 = 0, 1
# status codes of include/mpsengine.h
MPSE_OK, MPSE_ERR_OOM, MPSE_ERR_SHAPE, MPSE_ERR_NOCONV, MPSE_ERR_HIP, MPSE_ERR_ARG = 0, 1, 2, 3, 4, 5
DOMAIN_L, DOMAIN_R = 0, 1

STATUS = {0: "OK", 1: "OOM", 2: "SHAPE", 3: "NOCONV", 4: "HIP", 5: "ARG"}


PcgResult = collections.namedtuple("PcgResult", "status iters relres lvalue")


class EngineError(RuntimeError):
    pass


class DeviceMemoryError(EngineError, MemoryError):
    """Device allocation failure (the reference's MEMORY_ERRORS, mps/backend.py:89-94)."""


class mpse_index(C.Structure):
    _fields_ = [("ext", C.c_int64), ("lo_ext", C.c_int64), ("s_hi", C.c_int64), ("s_lo", C.c_int64)]


class mpse_gemm_desc(C.Structure):
    _fields_ = [("dtype_a", C.c_int), ("dtype_b", C.c_int), ("conj_a", C.c_int), ("conj_b", C.c_int),
                ("m_a", mpse_index), ("k_a", mpse_index), ("k_b", mpse_index), ("n_b", mpse_index),
                ("m_c", mpse_index), ("n_c", mpse_index),
                ("batch", C.c_int64), ("sb_a", C.c_int64), ("sb_b", C.c_int64), ("sb_c", C.c_int64),
                ("alpha_re", C.c_double), ("alpha_im", C.c_double), ("beta_re", C.c_double), ("beta_im", C.c_double),
                ("skip_zero_tiles", C.c_int)]


class mpse_dims(C.Structure):
    _fields_ = [("Dl_bra", C.c_int64), ("Dl_ket", C.c_int64), ("Dr_bra", C.c_int64), ("Dr_ket", C.c_int64),
                ("d0", C.c_int64), ("d1", C.c_int64), ("danc", C.c_int64),
                ("wl", C.c_int64), ("wm", C.c_int64), ("wr", C.c_int64), ("env_unit", C.c_int64),
                ("danc1", C.c_int64)]


class mpse_heff(C.Structure):
    _fields_ = [("nsite", C.c_int), ("dims", mpse_dims),
                ("L", C.c_void_p), ("l_dtype", C.c_int),
                ("R", C.c_void_p), ("r_dtype", C.c_int),
                ("W0", C.c_void_p), ("W1", C.c_void_p), ("w_dtype", C.c_int),
                ("l_unit", C.c_int64), ("r_unit", C.c_int64)]


LEG_UP, LEG_DOWN = 0, 1


class mpse_heff_ft(C.Structure):
    _fields_ = [("Dl", C.c_int64), ("Dr", C.c_int64), ("d_up", C.c_int64), ("d_down", C.c_int64),
                ("wl1", C.c_int64), ("wr1", C.c_int64), ("wl2", C.c_int64), ("wr2", C.c_int64),
                ("leg1", C.c_int), ("leg2", C.c_int), ("trans1", C.c_int), ("trans2", C.c_int),
                ("L", C.c_void_p), ("l_dtype", C.c_int),
                ("R", C.c_void_p), ("r_dtype", C.c_int),
                ("W1", C.c_void_p), ("W2", C.c_void_p), ("w_dtype", C.c_int)]


def idx1(ext, stride):
    return mpse_index(int(ext), max(int(ext), 1), 0, int(stride))


def idx2(hi, lo, s_hi, s_lo):
    return mpse_index(int(hi) * int(lo), max(int(lo), 1), int(s_hi), int(s_lo))


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float64:
        return F64
    if dt == np.complex128:
        return C128
    raise TypeError(f"unsupported dtype {dt}; the engine computes in float64 / complex128")


_i64p = C.POINTER(C.c_int64)
_dblp = C.POINTER(C.c_double)

_SIGNATURES = {
    "mpse_ctx_create": [C.c_int, C.POINTER(C.c_void_p)],
    "mpse_ctx_destroy": [C.c_void_p],
    "mpse_sync": [C.c_void_p],
    "mpse_device_info": [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_void_p)],
    "mpse_prof_enable": [C.c_void_p, C.c_int],
    "mpse_prof_reset": [C.c_void_p],
    "mpse_prof_get": [C.c_void_p, C.c_int, _dblp, _dblp, _dblp, C.POINTER(C.c_int64)],
    "mpse_prof_get_ktiles": [C.c_void_p, C.c_int, C.POINTER(C.c_int64)],
    "mpse_prof_get_svd_sweeps": [C.c_void_p, C.POINTER(C.c_int64)],
    "mpse_mpo_site_hint": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64],
    "mpse_block_qr_stats": [C.c_void_p] + [C.POINTER(C.c_int64)] * 3,
    "mpse_heff_fused_stats": [C.c_void_p] + [C.POINTER(C.c_int64)] * 2,
    "mpse_block_qr_optimistic": [C.c_void_p, C.c_int],
    "mpse_block_qr_scheme": [C.c_void_p, C.c_int],
    "mpse_block_qr_check": [C.c_void_p, C.POINTER(C.c_int)],
    "mpse_block_qr_pass_stats": [C.c_void_p] + [C.POINTER(C.c_int64)] * 2,
    "mpse_block_qr_path_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_malloc": [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)],
    "mpse_free": [C.c_void_p, C.c_void_p],
    "mpse_pool_trim": [C.c_void_p],
    "mpse_mem_info": [C.c_void_p] + [C.POINTER(C.c_size_t)] * 4,
    "mpse_memcpy_h2d": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "mpse_memcpy_d2h": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "mpse_memcpy_d2d": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "mpse_memset_zero": [C.c_void_p, C.c_void_p, C.c_size_t],
    "mpse_memcpy_2d": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t],
    "mpse_cast_f64_to_c128": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_conj_inplace": [C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_scal": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.c_double],
    "mpse_axpy": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double],
    "mpse_mul_real": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_davidson_precond": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                              C.c_double, C.c_double],
    "mpse_real_part": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_dotc": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _dblp],
    "mpse_nrm2": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, _dblp],
    "mpse_scaled_rms": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, _dblp],
    "mpse_expm_centre_mask": [C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_solve_slot": [C.c_void_p, C.c_int64],
    "mpse_plan_store_budget": [C.c_void_p, C.c_int64],
    "mpse_plan_reuse_stats": [C.c_void_p, C.POINTER(C.c_int64), C.c_int],
    "mpse_defer_begin": [C.c_void_p, C.c_int],
    "mpse_defer_end": [C.c_void_p],
    "mpse_defer_arm": [C.c_void_p, C.c_int],
    "mpse_defer_run": [C.c_void_p, C.c_int],
    "mpse_defer_discard": [C.c_void_p],
    "mpse_gemm": [C.c_void_p, C.POINTER(mpse_gemm_desc), C.c_void_p, C.c_void_p, C.c_void_p],
    "mpse_gemm_path_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_transpose_inner": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int],
    "mpse_env_update": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_dims), C.c_void_p, C.c_int, C.c_void_p,
                        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p],
    "mpse_heff_apply": [C.c_void_p, C.c_int, C.POINTER(mpse_heff), C.c_void_p, C.c_void_p],
    "mpse_heff_apply2": [C.c_void_p, C.c_int, C.POINTER(mpse_heff), C.c_void_p, C.c_void_p],
    "mpse_env_update_multi": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_dims), C.c_int, _i64p, _i64p, C.c_void_p,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_void_p],
    "mpse_env_unit_channel": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_double, _i64p],
    "mpse_expm_lanczos": [C.c_void_p, C.c_int, C.POINTER(mpse_heff), C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                          C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int)],
    "mpse_expm_lanczos_batch": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_heff), C.c_double, C.c_double,
                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double, C.c_double, C.c_int,
                                C.POINTER(C.c_int)],
    "mpse_expm_lanczos_batch_stats": [C.c_void_p, _i64p, _i64p],
    "mpse_expm_lanczos_path_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_davidson": [C.c_void_p, C.c_int, C.POINTER(mpse_heff), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                      C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, _dblp, C.c_void_p,
                      C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "mpse_pcg": [C.c_void_p, C.c_int, C.POINTER(mpse_heff), C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int), _dblp, _dblp],
    "mpse_pcg_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_pcg_batch": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_heff), C.c_int, _dblp, C.POINTER(C.c_void_p),
                       C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double, C.c_int,
                       C.POINTER(C.c_int), C.POINTER(C.c_int), _dblp, _dblp],
    "mpse_pcg_batch_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_pcg_batch_plan": [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _i64p, C.c_int],
    "mpse_heff_apply_ft": [C.c_void_p, C.c_int, C.POINTER(mpse_heff_ft), C.c_void_p, C.c_void_p],
    "mpse_env_update_ft": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_heff_ft), C.c_void_p, C.c_int, C.c_void_p,
                           C.c_void_p],
    "mpse_pcg_sum": [C.c_void_p, C.c_int, C.c_int, C.POINTER(mpse_heff_ft), _dblp, C.c_double, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int), _dblp, _dblp],
    "mpse_pcg_sum_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_site_factor_ft": [C.c_void_p, C.POINTER(mpse_heff_ft), C.c_void_p],
    "mpse_diag_ft": [C.c_void_p, C.POINTER(mpse_heff_ft), C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p],
    "mpse_mps_overlap": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                         C.POINTER(C.c_int), _i64p, C.c_int, _dblp],
    "mpse_mps_overlap_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_overlap_plan": [C.c_int, _i64p, C.c_int, _i64p, C.c_int],
    "mpse_mps_sandwich": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                          C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int, _dblp],
    "mpse_mps_sandwich_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_sandwich_plan": [C.c_int, _i64p, C.c_int, _i64p, C.c_int],
    "mpse_mps_corr": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int, C.POINTER(C.c_int),
                      _dblp, _dblp, _dblp, _dblp],
    "mpse_mps_corr_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_corr_plan": [C.c_int, _i64p, C.c_int, C.c_int, _i64p, C.c_int],
    "mpse_mps_rdm1": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int, C.POINTER(C.c_int),
                      _dblp],
    "mpse_mps_rdm1_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_rdm1_plan": [C.c_int, _i64p, C.c_int, C.c_int, _i64p, C.c_int],
    "mpse_mps_rdm2": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int, C.POINTER(C.c_int),
                      _dblp],
    "mpse_mps_rdm2_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_rdm2_plan": [C.c_int, _i64p, C.c_int, C.POINTER(C.c_int), C.c_int, _i64p, C.c_int],
    "mpse_mps_trdm1": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                       C.POINTER(C.c_int), _i64p, C.c_int, C.c_int, C.POINTER(C.c_int), _dblp],
    "mpse_mps_trdm1_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_trdm1_plan": [C.c_int, _i64p, C.c_int, C.c_int, _i64p, C.c_int],
    "mpse_mps_bond_spectra": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int,
                              C.POINTER(C.c_int), _dblp],
    "mpse_mps_bond_spectra_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_bond_spectra_plan": [C.c_int, _i64p, C.c_int, C.c_int, _i64p, C.c_int],
    "mpse_mps_expect_many": [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p, C.c_int,
                             C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int), _i64p,
                             _dblp],
    "mpse_mps_expect_many_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_mps_expect_many_plan": [C.c_int, _i64p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _i64p, C.c_int,
                                  _i64p, C.c_int],
    "mpse_truncate_select": [_dblp, _i64p, C.c_int64, C.c_int64, C.c_double, _i64p, _i64p],
    "mpse_block_qr": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, _i64p, _i64p, _i64p, _i64p,
                      C.c_int, C.c_void_p, C.c_void_p, C.c_int64],
    "mpse_block_svd": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, _i64p, _i64p, _i64p, _i64p,
                       C.c_void_p, C.c_void_p, _dblp, C.c_int64],
    "mpse_block_svd_full": [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, _i64p, _i64p, _i64p, _i64p,
                            _i64p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, _dblp, C.c_int64],
    "mpse_block_svd_stats": [C.c_void_p, _i64p, C.c_int],
    "mpse_gather_cols": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _i64p, _dblp, C.c_int64],
    "mpse_gather_rows": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _i64p, _dblp, C.c_int64],
    "mpse_tda_create": [C.c_void_p, C.c_int] + [C.POINTER(C.c_void_p), C.POINTER(C.c_int)] * 4 +
                       [_i64p, C.POINTER(C.c_void_p), _i64p, C.POINTER(C.c_int)],
    "mpse_tda_destroy": [C.c_void_p, C.c_void_p],
    "mpse_tda_apply": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "mpse_tda_hdiag": [C.c_void_p, C.c_void_p, C.c_void_p],
    "mpse_tda_davidson": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                          C.c_int, C.c_int, C.c_double, C.c_double, _dblp, C.c_void_p, C.POINTER(C.c_int),
                          C.POINTER(C.c_int)],
    "mpse_tda_stats": [C.c_void_p, _i64p, C.c_int],
}
EXPORTED_SYMBOLS = sorted(list(_SIGNATURES) + ["mpse_last_error", "mpse_version"])


def load_library(path=LIB_PATH):
    """dlopen the HIP engine and attach prototypes.  Raises EngineError if it is not built."""
    if not os.path.exists(path):
        raise EngineError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  renormalizer_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.mpse_last_error.argtypes = [C.c_void_p]
    lib.mpse_last_error.restype = C.c_char_p
    lib.mpse_version.argtypes = []
    lib.mpse_version.restype = C.c_char_p
    return lib


def _chain_plan(lib_fn, dims, row_len, row, info_names, *extra):
    """(chain kernel?, {info name: value}) of one of the ``mpse_mps_*_plan`` exports for the ``dims`` rows of ``row_len``
    extents, which ``row`` names; ``extra``: the arguments between the table and the info array"""
    rows = [[int(x) for x in r] for r in dims]
    assert all(len(r) == row_len for r in rows), f"dims rows are ({row})"
    flat = (C.c_int64 * max(row_len * len(rows), 1))(*[x for r in rows for x in r])
    info = (C.c_int64 * len(info_names))()
    ok = lib_fn(len(rows), flat, *extra, info, len(info))
    return bool(ok), dict(zip(info_names, (int(v) for v in info)))


OVERLAP_PLAN_INFO = ("bond_limit", "lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "max_bond", "valid")


def mps_overlap_plan(dims, any_complex, lib=None):
    """Which path ``Engine.mps_overlap`` takes for a chain, from its ``dims`` rows (Db_l, Dk_l, p, Db_r, Dk_r) alone
    (``mpse_mps_overlap_plan``; needs the built library, no GPU).  Returns (chain kernel?, {info name: value})."""
    return _chain_plan((lib or load_library()).mpse_mps_overlap_plan, dims, 5, "Db_l, Dk_l, p, Db_r, Dk_r",
                       OVERLAP_PLAN_INFO, int(bool(any_complex)))


SANDWICH_PLAN_INFO = ("lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "acc_per_thread", "acc_needed",
                      "work_max", "work", "valid", "elem_bytes", "channel_limit")


def mps_sandwich_plan(dims, any_complex, lib=None):
    """Which path ``Engine.mps_sandwich`` takes for a chain, from its ``dims`` rows (Db_l, Dk_l, wl, d, danc, Db_r,
    Dk_r, wr) alone (``mpse_mps_sandwich_plan``; needs the built library, no GPU).  Returns (chain kernel?, {info name:
    value})."""
    return _chain_plan((lib or load_library()).mpse_mps_sandwich_plan, dims, 8,
                       "Db_l, Dk_l, wl, d, danc, Db_r, Dk_r, wr", SANDWICH_PLAN_INFO, int(bool(any_complex)))


CORR_PLAN_INFO = ("bond_limit", "lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "max_bond", "valid",
                  "nsel_limit", "p_limit", "bond_fit_limit", "lds_fit_bytes")


def mps_corr_plan(dims, nsel, any_complex, lib=None):
    """Which path ``Engine.mps_corr`` takes for a chain, from its ``dims`` rows (D_l, d, danc, D_r) and the number of
    selected sites alone (``mpse_mps_corr_plan``; needs the built library, no GPU).  Returns (chain kernels?, {info
    name: value})."""
    return _chain_plan((lib or load_library()).mpse_mps_corr_plan, dims, 4, "D_l, d, danc, D_r", CORR_PLAN_INFO,
                       int(nsel), int(bool(any_complex)))


RDM1_PLAN_INFO = ("bond_limit", "lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "max_bond", "valid",
                  "nsel_limit", "p_limit", "bond_fit_limit", "lds_fit_bytes")


def mps_rdm1_plan(dims, nsel, any_complex, lib=None):
    """Which path ``Engine.mps_rdm1`` takes for a chain, from its ``dims`` rows (D_l, d, danc, D_r) and the number of
    selected sites alone (``mpse_mps_rdm1_plan``; needs the built library, no GPU).  Returns (chain kernels?, {info
    name: value}); ``nsel_limit`` is 0: the kernels take any number of selected sites."""
    return _chain_plan((lib or load_library()).mpse_mps_rdm1_plan, dims, 4, "D_l, d, danc, D_r", RDM1_PLAN_INFO,
                       int(nsel), int(bool(any_complex)))


RDM2_PLAN_INFO = RDM1_PLAN_INFO + ("units", "out_elems", "stack_bytes")


def mps_rdm2_plan(dims, sel, any_complex, lib=None):
    """Which path ``Engine.mps_rdm2`` takes for a chain, from its ``dims`` rows (D_l, d, danc, D_r) and the selected
    sites alone (``mpse_mps_rdm2_plan``; needs the built library, no GPU).  Returns (chain kernels?, {info name:
    value}); ``units``: the workgroups of the second launch, ``out_elems``: the complex elements of the result (both 0
    for a table or a selection the call refuses), ``stack_bytes``: the byte bound of a chunk of the enqueued path."""
    sel = [int(k) for k in sel]
    return _chain_plan((lib or load_library()).mpse_mps_rdm2_plan, dims, 4, "D_l, d, danc, D_r", RDM2_PLAN_INFO,
                       len(sel), (C.c_int * max(len(sel), 1))(*sel), int(bool(any_complex)))


TRDM1_PLAN_INFO = ("bond_limit", "lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "max_bond_bra",
                   "max_bond_ket", "valid", "nsel_limit", "p_limit", "acc_limit", "lds_fit_bytes", "bond_limit_bra1")


def mps_trdm1_plan(dims, nsel, any_complex, lib=None):
    """Which path ``Engine.mps_trdm1`` takes for two chains, from their ``dims`` rows (Db_l, Dk_l, d, danc, Db_r, Dk_r)
    and the number of selected sites alone (``mpse_mps_trdm1_plan``; needs the built library, no GPU).  Returns (chain
    kernels?, {info name: value}); ``acc_limit``: the largest Db * Dk of a bond the launches take, ``bond_limit_bra1``:
    the rule's limit for the ket when every bond of the bra is 1."""
    return _chain_plan((lib or load_library()).mpse_mps_trdm1_plan, dims, 6, "Db_l, Dk_l, d, danc, Db_r, Dk_r",
                       TRDM1_PLAN_INFO, int(nsel), int(bool(any_complex)))


BOND_SPECTRA_PLAN_INFO = RDM1_PLAN_INFO + ("eig_elems", "sweep_cap")


def mps_bond_spectra_plan(dims, nsel, any_complex, lib=None):
    """Which path ``Engine.mps_bond_spectra`` takes for a chain, from its ``dims`` rows (D_l, d, danc, D_r) and the
    number of selected bonds alone (``mpse_mps_bond_spectra_plan``; needs the built library, no GPU).  Returns (chain
    kernels?, {info name: value}); ``eig_elems``: the LDS elements of the eigensolver launch, 2 D (D | 1) + D at the
    largest bond D of the table, ``sweep_cap``: the sweeps after which a Jacobi solve fails the call; ``lds_bytes`` and
    ``lds_fit_bytes`` are those of the larger of the two launches."""
    return _chain_plan((lib or load_library()).mpse_mps_bond_spectra_plan, dims, 4, "D_l, d, danc, D_r",
                       BOND_SPECTRA_PLAN_INFO, int(nsel), int(bool(any_complex)))


EXPECT_MANY_PLAN_INFO = ("bond_limit", "lds_budget", "lds_bytes", "e_elems", "t_elems", "threads", "max_bond", "valid",
                         "grid_cap", "p_limit", "bond_fit_limit", "lds_fit_bytes", "win_e_elems", "win_t_elems", "w_max",
                         "channel_limit", "acc_needed", "acc_per_thread", "elem_bytes")


def _window_args(windows):
    """(nop, first array, last array, wdims array) of ``windows``: one (first site, [(wl, wr) per MPO site]) per
    operator"""
    nop = len(windows)
    first = [int(f) for f, _ in windows]
    last = [int(f) + len(w) - 1 for f, w in windows]
    flat = [int(x) for _, w in windows for pair in w for x in pair]
    return (nop, (C.c_int * max(nop, 1))(*first), (C.c_int * max(nop, 1))(*last),
            (C.c_int64 * max(len(flat), 2))(*flat))


def mps_expect_many_plan(dims, windows, any_complex, lib=None):
    """Which path ``Engine.mps_expect_many`` takes, from the ``dims`` rows (D_l, d, danc, D_r) of the chain and the
    ``windows`` of the operators alone, one (first site, [(wl, wr) per MPO site of the window]) each
    (``mpse_mps_expect_many_plan``; needs the built library, no GPU).  Returns (chain kernels?, {info name: value});
    ``valid``: the table is a chain AND every window lies inside it with MPO bonds from 1 to 1 (a window without sites
    stands for first > last), ``grid_cap``: the workgroups of one launch of the window kernel, ``lds_bytes`` and
    ``lds_fit_bytes``: the larger of the two launches."""
    return _chain_plan((lib or load_library()).mpse_mps_expect_many_plan, dims, 4, "D_l, d, danc, D_r",
                       EXPECT_MANY_PLAN_INFO, *_window_args(windows), int(bool(any_complex)))


def check_selection(call, sel, nsite):
    """The site selection of a chain call as a list of ints; ValueError unless it is strictly ascending inside
    [0, nsite) and not empty"""
    sel = [int(k) for k in sel]
    if not sel or sel[0] < 0 or sel[-1] >= nsite or any(b <= a for a, b in zip(sel, sel[1:])):
        raise ValueError(f"{call}: the selection {sel} is not strictly ascending inside [0, {nsite})")
    return sel


def _site_args(sites):
    """(pointer array, dtype-code array) of a list of device site tensors, as the chain calls take them"""
    n = len(sites)
    return (C.c_void_p * n)(*[t.ptr for t in sites]), (C.c_int * n)(*[t.code for t in sites])


class _Recording:
    def __init__(self, eng, which):
        self.eng, self.which = eng, which

    def __enter__(self):
        self.eng._check(self.eng.lib.mpse_defer_begin(self.eng.ctx, self.which))
        self.eng.recording_list = self.which
        return self

    def __exit__(self, et, ev, tb):
        self.eng.recording_list = -1
        if et is None:
            self.eng._check(self.eng.lib.mpse_defer_end(self.eng.ctx))
        else:
            self.eng.lib.mpse_defer_discard(self.eng.ctx)
        return False


class _Buffer:
    """Owns one pooled device allocation."""
    __slots__ = ("eng", "ptr", "nbytes", "__weakref__")

    def __init__(self, eng, nbytes):
        self.eng = eng
        self.nbytes = int(nbytes)
        self.ptr = None                     # stays None if the allocation below raises (see __del__)
        p = C.c_void_p()
        eng._check(eng.lib.mpse_malloc(eng.ctx, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value

    def __del__(self):
        eng = self.eng
        if eng is not None and eng.ctx is not None and self.ptr:
            try:
                eng.lib.mpse_free(eng.ctx, self.ptr)
            except Exception:
                pass
            self.ptr = None


class DeviceTensor:
    """Dense C-ordered float64 / complex128 tensor resident in HBM.

    Plays the role of the reference's ``Matrix`` (mps/matrix.py:13-186) except that the
    data never lives on the host: slicing-free, reshape is a free view, ``to_host``
    is the only PCIe crossing."""
    __slots__ = ("eng", "buf", "offset", "shape", "dtype", "sigmaqn", "unit")

    def __init__(self, eng, buf, offset, shape, dtype):
        self.eng = eng
        self.buf = buf
        self.offset = int(offset)
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.sigmaqn = None
        self.unit = 0       # environments only: 1-based MPO channel that is the identity matrix (mpse_env_unit_channel)

    # -- basic properties
    @property
    def ptr(self):
        return self.buf.ptr + self.offset

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return math.prod(self.shape)

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def code(self):
        return dtype_code(self.dtype)

    @property
    def is_complex(self):
        return self.dtype == np.complex128

    # shape helpers of the reference's Matrix (mps/matrix.py:66-91): a site tensor is (left bond, physical.., right bond)
    @property
    def pdim(self):
        return self.shape[1:-1]

    @property
    def pdim_prod(self):
        return int(np.prod(self.shape[1:-1]))

    @property
    def bond_dim(self):
        return self.shape[0], self.shape[-1]

    @property
    def r_combine_shape(self):
        return self.shape[0], int(np.prod(self.shape[1:]))

    @property
    def l_combine_shape(self):
        return int(np.prod(self.shape[:-1])), self.shape[-1]

    def r_combine(self):
        return self.reshape(self.r_combine_shape)

    def l_combine(self):
        return self.reshape(self.l_combine_shape)

    @property
    def array(self):
        """Host copy (the reference's ``Matrix.array``)."""
        return self.to_host()

    def __repr__(self):
        return f"DeviceTensor(shape={self.shape}, dtype={self.dtype})"

    # -- views / copies
    def reshape(self, *shape):
        if len(shape) == 1 and not isinstance(shape[0], (int, np.integer)):
            shape = tuple(shape[0])
        shape = [int(s) for s in shape]
        size = math.prod(self.shape)
        if -1 in shape:
            i = shape.index(-1)
            rest = math.prod(s for s in shape if s != -1)
            shape[i] = size // rest if rest else 0
        if math.prod(shape) != size:
            raise ValueError(f"cannot reshape {self.shape} into {tuple(shape)}")
        return DeviceTensor(self.eng, self.buf, self.offset, shape, self.dtype)

    def ravel(self):
        return self.reshape(self.size)

    def row_block(self, start, stop):
        """View of rows [start, stop) along the first axis (contiguous)."""
        inner = math.prod(self.shape[1:]) * self.dtype.itemsize
        return DeviceTensor(self.eng, self.buf, self.offset + start * inner, (stop - start,) + self.shape[1:], self.dtype)

    def shifted(self, nelem):
        """Flat view of the same buffer starting ``nelem`` elements further on (operand offsets of strided GEMMs)."""
        return DeviceTensor(self.eng, self.buf, self.offset + int(nelem) * self.dtype.itemsize,
                            (self.size - int(nelem),), self.dtype)

    def copy(self):
        out = self.eng.empty(self.shape, self.dtype)
        self.eng._check(self.eng.lib.mpse_memcpy_d2d(self.eng.ctx, out.ptr, self.ptr, self.nbytes))
        return out

    def to_complex(self):
        if self.is_complex:
            return self
        out = self.eng.empty(self.shape, np.complex128)
        self.eng._check(self.eng.lib.mpse_cast_f64_to_c128(self.eng.ctx, out.ptr, self.ptr, self.size))
        return out

    def conj(self):
        if not self.is_complex:
            return self
        out = self.copy()
        self.eng._check(self.eng.lib.mpse_conj_inplace(self.eng.ctx, out.ptr, out.size))
        return out

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.size:
            self.eng._check(self.eng.lib.mpse_memcpy_d2h(self.eng.ctx, out.ctypes.data, self.ptr, self.nbytes))
        return out

    # -- in-place scalar algebra used by the sweeps
    def scale_(self, a):
        a = complex(a)
        if a.imag != 0 and not self.is_complex:
            raise TypeError("complex scale of a real tensor")
        self.eng._check(self.eng.lib.mpse_scal(self.eng.ctx, self.code, self.ptr, self.size, a.real, a.imag))
        return self

    def norm(self):
        out = (C.c_double * 2)()
        self.eng._check(self.eng.lib.mpse_nrm2(self.eng.ctx, self.code, self.ptr, self.size, out))
        return float(out[0])

    def vdot(self, other):
        """sum conj(self) * other"""
        assert other.dtype == self.dtype and other.size == self.size
        out = (C.c_double * 2)()
        self.eng._check(self.eng.lib.mpse_dotc(self.eng.ctx, self.code, self.ptr, other.ptr, self.size, out))
        return complex(out[0], out[1]) if self.is_complex else float(out[0])


class TdaOperator:
    """The Hamiltonian projected onto the first-order tangent space of a matrix product state (``mpse_tda_*``,
    include/mpsengine.h): ``a``, ``b`` the left- / right-canonical device sites (Dl, d, Dr), ``u`` the tangent factors
    (Dl, d, n) or None, ``w`` the MPO sites (wl, d, d, wr).  The engine handle borrows the tensors; this object keeps
    them alive.  ``dtype`` is the working dtype of the vectors, ``xsize`` their length."""

    def __init__(self, eng, a, b, u, w):
        n = len(a)
        if not (len(b) == len(u) == len(w) == n) or n < 1:
            raise ValueError("TdaOperator: a, b, u, w must list the same sites")
        self.eng = eng
        self.handle = None
        self._keep = (list(a), list(b), list(u), list(w))
        rows = []
        for i in range(n):
            if a[i].ndim != 3 or w[i].ndim != 4 or a[i].shape != b[i].shape:
                raise ValueError(f"TdaOperator: site {i}: A {a[i].shape}, B {b[i].shape}, W {w[i].shape}")
            if u[i] is not None and (u[i].ndim != 3 or u[i].shape[:2] != a[i].shape[:2]):
                raise ValueError(f"TdaOperator: site {i}: U {u[i].shape} on a site {a[i].shape}")
            rows += [a[i].shape[0], a[i].shape[1], a[i].shape[2], w[i].shape[0], w[i].shape[3],
                     0 if u[i] is None else u[i].shape[2]]
            if w[i].shape[1:3] != (a[i].shape[1],) * 2:
                raise ValueError(f"TdaOperator: site {i}: W {w[i].shape} on a site {a[i].shape}")
        self.xshape = [None if u[i] is None else (u[i].shape[2], b[i].shape[2]) for i in range(n)]
        uptr = (C.c_void_p * n)(*[None if t is None else t.ptr for t in u])
        ucode = (C.c_int * n)(*[0 if t is None else t.code for t in u])
        h, xs, dt = C.c_void_p(), C.c_int64(), C.c_int()
        eng._check(eng.lib.mpse_tda_create(eng.ctx, n, *_site_args(a), *_site_args(b), uptr, ucode, *_site_args(w),
                                           (C.c_int64 * len(rows))(*rows), C.byref(h), C.byref(xs), C.byref(dt)))
        self.handle = h.value
        self.xsize = int(xs.value)
        self.dtype = np.dtype(np.complex128 if dt.value == C128 else np.float64)

    def close(self):
        if self.handle and self.eng.ctx is not None:
            self.eng.lib.mpse_tda_destroy(self.eng.ctx, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, x, y=None):
        """y = P^H H P x for a device vector of ``xsize`` elements of ``dtype``; enqueued, no host synchronisation"""
        if x.dtype != self.dtype or x.size != self.xsize:
            raise ValueError(f"TdaOperator.apply: x {x.shape} {x.dtype}, the operator takes {self.xsize} of {self.dtype}")
        if y is None:
            y = self.eng.empty((self.xsize,), self.dtype)
        self.eng._check(self.eng.lib.mpse_tda_apply(self.eng.ctx, self.handle, x.ptr, y.ptr))
        return y

    def hdiag(self):
        """Re diag(P^H H P) as a float64 device vector (the Davidson preconditioner)"""
        out = self.eng.empty((self.xsize,), np.float64)
        self.eng._check(self.eng.lib.mpse_tda_hdiag(self.eng.ctx, self.handle, out.ptr))
        return out

    def davidson(self, guesses, hdiag, nroots, tol=1e-12, max_cycle=100, max_space=None, lindep=1e-14, shift=1e-4):
        """The ``nroots`` lowest eigenpairs by the engine's Davidson (``mpse_tda_davidson``); ``guesses``: host arrays of
        ``xsize`` elements.  Returns (e (nroots,), x (nroots, xsize) host array, ncycle, nmatvec)."""
        eng = self.eng
        g = eng.asdevice(np.ascontiguousarray(np.stack([np.asarray(v).reshape(-1) for v in guesses]), dtype=self.dtype))
        if g.shape[1] != self.xsize:
            raise ValueError(f"TdaOperator.davidson: guesses of {g.shape[1]} elements, the operator takes {self.xsize}")
        out = eng.empty((nroots, self.xsize), self.dtype)
        e = (C.c_double * nroots)()
        ncyc, nmv = C.c_int(), C.c_int()
        eng._check(eng.lib.mpse_tda_davidson(eng.ctx, g.code, self.handle, hdiag.ptr, nroots, g.shape[0], g.ptr, tol,
                                             max_cycle, 0 if max_space is None else max_space, lindep, shift, e,
                                             out.ptr, C.byref(ncyc), C.byref(nmv)))
        return np.array([float(v) for v in e]), out.to_host(), ncyc.value, nmv.value


class Engine:
    """One HIP context (device + stream + memory pool) per process, as in the
    reference's single-GPU backend (mps/backend.py:129-132)."""

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("RENO_GPU", "0"))
        self.lib = load_library()
        self.ctx = None
        p = C.c_void_p()
        st = self.lib.mpse_ctx_create(int(device), C.byref(p))
        if st != 0:
            raise EngineError(
                f"mpse_ctx_create(device={device}) failed with status {STATUS.get(st, st)}: no usable MI355X/HIP "
                "device.  renormalizer_amd has no CPU fallback.")
        self.ctx = p.value
        self.device = int(device)
        name = C.create_string_buffer(128)
        ncu = C.c_int()
        stream = C.c_void_p()
        self.lib.mpse_device_info(self.ctx, name, 128, C.byref(ncu), C.byref(stream))
        self.device_name = name.value.decode()
        self.n_cu = ncu.value
        self.stream = stream.value
        self._ones = {}
        self.recording_list = -1            # list being recorded (mpse_defer_begin), -1 = none

    def close(self):
        if self.ctx is not None:
            self.lib.mpse_ctx_destroy(self.ctx)
            self.ctx = None

    # -- status handling
    def _check(self, st):
        if st == 0:
            return
        msg = self.lib.mpse_last_error(self.ctx)
        msg = msg.decode() if msg else ""
        if st == 1:
            raise DeviceMemoryError(f"device out of memory: {msg}")
        if st == 2:
            raise ValueError(f"mpsengine: {msg}")
        raise EngineError(f"mpsengine status {STATUS.get(st, st)}: {msg}")

    def sync(self):
        self._check(self.lib.mpse_sync(self.ctx))

    # -- deferred calls (mpse_defer_*): gemm / block QR / environment updates issued inside ``recording(list)`` are
    # stored and run at the end of the Lanczos solve that follows ``arm(list)``
    def recording(self, which):
        return _Recording(self, which)

    def arm(self, which):
        self._check(self.lib.mpse_defer_arm(self.ctx, which))

    def defer_discard(self):
        self.recording_list = -1
        self.lib.mpse_defer_discard(self.ctx)

    def mem_info(self):
        v = [C.c_size_t() for _ in range(4)]
        self._check(self.lib.mpse_mem_info(self.ctx, *[C.byref(x) for x in v]))
        return dict(pool=v[0].value, in_use=v[1].value, device_free=v[2].value, device_total=v[3].value)

    def free_all_blocks(self):
        self._check(self.lib.mpse_pool_trim(self.ctx))

    def mpo_site_hint(self, dev, host):
        """Describe a real MPO site to the engine (``mpse_mpo_site_hint``): ``dev`` is the device copy of ``host``
        (wl, d, d, wr).  Large one-site matvecs on that site then take the folded plan.  The hint goes with the
        buffer, and these entry points drop it when they write into the described range: ``mpse_memcpy_h2d``,
        ``mpse_memcpy_d2d``, ``mpse_memcpy_2d``, ``mpse_memset_zero``, ``mpse_scal``, ``mpse_conj_inplace``,
        ``mpse_axpy``, ``mpse_mul_real``, ``mpse_real_part``, ``mpse_cast_f64_to_c128``, ``mpse_davidson_precond``,
        ``mpse_gather_cols``, ``mpse_gather_rows``, ``mpse_transpose_inner`` and the solution vectors of ``mpse_pcg``,
        ``mpse_pcg_sum`` and ``mpse_pcg_batch``.  Any other writer (GEMM and contraction results, the factors of a
        decomposition, the outputs of the other solvers) must not target a described buffer."""
        host = np.asarray(host)
        if host.ndim != 4 or np.iscomplexobj(host) or dev.is_complex or dev.offset != 0:
            return
        w = np.ascontiguousarray(host, dtype=np.float64)
        self._check(self.lib.mpse_mpo_site_hint(self.ctx, dev.ptr, w.ctypes.data, *[int(x) for x in w.shape[:2]],
                                                int(w.shape[3])))

    # -- kernel profiling (HIP events on the engine stream)
    def prof_enable(self, on=True):
        """on: False/0 off, True/1 every launch, N > 1 every N-th launch."""
        self._check(self.lib.mpse_prof_enable(self.ctx, int(on)))

    def prof_reset(self):
        self._check(self.lib.mpse_prof_reset(self.ctx))

    def _stats_dict(self, fn, names):
        """{name: count} of one of the ``*_stats`` exports that fill an array of counters in the order of ``names``"""
        v = (C.c_int64 * len(names))()
        self._check(fn(self.ctx, v, len(v)))
        return dict(zip(names, (int(x) for x in v)))

    def lanczos_batch_stats(self):
        """(members solved by the batched Krylov kernels, members of mpse_expm_lanczos_batch calls that took the single
        solve), cumulative"""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.mpse_expm_lanczos_batch_stats(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    LANCZOS_PATHS = ("sync", "async_done", "host_first", "host_later", "limit", "breakdown_async", "breakdown_sync",
                     "full_space", "converged", "noconv", "merged_first", "host_waits", "basis_growths", "update_parts",
                     "update_vmask", "update_unvec", "rescaled", "alias_restart")

    def lanczos_path_stats(self):
        """{path: count}: how the Lanczos solves of this context ran, cumulative (``mpse_expm_lanczos_path_stats``;
        the names follow the order of include/mpsengine.h)."""
        return self._stats_dict(self.lib.mpse_expm_lanczos_path_stats, self.LANCZOS_PATHS)

    PCG_STATS = ("solves", "iterations", "matvecs", "host_waits", "end_tol", "end_max_iter", "end_curvature",
                 "twolayer", "masked", "wait_interval")

    def pcg_stats(self):
        """{name: count}: what the conjugate-gradient solves of this context did, cumulative (``mpse_pcg_stats``; the
        names follow the order of include/mpsengine.h).  ``wait_interval`` is no count: the engine's number of
        iterations between two host reads of the control block."""
        return self._stats_dict(self.lib.mpse_pcg_stats, self.PCG_STATS)

    def pcg(self, hop, b, x, diag=None, mask=None, shift=0.0, tol=1e-5, max_iter=0, check=True):
        """Solve ``(mask * hop + shift) x = b`` by preconditioned conjugate gradients inside the engine (``mpse_pcg``).
        ``hop``: a ``hop_expr`` closure of a Hermitian positive definite operator (``twolayer`` is taken from it);
        ``b`` and ``x`` device tensors of the working dtype, ``x`` holds the start vector and receives the solution;
        ``diag`` (float64 device tensor, ``shift`` included) the preconditioner, ``mask`` (float64 0/1) the
        symmetry-allowed entries.  Returns ``PcgResult(status, iters, relres, lvalue)``; status 3 (not converged
        within ``max_iter``) is returned, any other failure raises unless ``check`` is False."""
        self._pcg_operands(int(np.prod(hop.cshape)), b, x, diag, mask)
        it, rel, lv = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        st = self.lib.mpse_pcg(self.ctx, x.code, C.byref(hop.heff), int(hop.twolayer), float(shift),
                               None if diag is None else diag.ptr, None if mask is None else mask.ptr, b.ptr, x.ptr,
                               float(tol), int(max_iter), C.byref(it), C.byref(rel), C.byref(lv))
        return self._pcg_result(st, it.value, rel.value, lv.value, check)

    @staticmethod
    def _pcg_operands(n, b, x, diag, mask):
        """the operands of one conjugate-gradient system against its length ``n``"""
        assert b.size == n and x.size == n and b.dtype == x.dtype, (b.shape, x.shape, n)
        assert diag is None or (diag.size == n and diag.dtype == np.float64)
        assert mask is None or (mask.size == n and mask.dtype == np.float64)

    def _pcg_result(self, st, iters, relres, lvalue, check=False):
        """``PcgResult`` from the outputs of a solve; ``check``: any status but 0 and 3 (not converged) raises"""
        if check and st not in (0, 3):
            self._check(st)
        return PcgResult(int(st), int(iters), float(relres), float(lvalue))

    PCG_BATCH_STATS = ("batched_members", "single_members", "launch_sets", "matvec_launches", "host_waits",
                       "set_limit")

    def pcg_batch_stats(self):
        """{name: count} of the ``pcg_batch`` calls of this context, cumulative (``mpse_pcg_batch_stats``; the names
        follow the order of include/mpsengine.h).  ``set_limit`` is no count: the member limit per launch set."""
        return self._stats_dict(self.lib.mpse_pcg_batch_stats, self.PCG_BATCH_STATS)

    def pcg_batch(self, hops, bs, xs, diags, masks, shifts, tol, max_iter=0):
        """``pcg`` for several independent systems in one call (``mpse_pcg_batch``): lists of ``hop_expr`` closures (all
        two-layer or all one-layer), right-hand sides, start vectors / solutions of one working dtype, preconditioner
        diagonals and masks (the list or single entries may be None) and shifts.  Two-layer one-site members whose
        shape passes ``small2_eligible`` are solved together, the others through ``mpse_pcg``; a member's result does
        not depend on the others.  Returns one ``PcgResult`` per member; a member's status is its own (0, 3 = not
        converged, 1 = refused), only a failure of the call as a whole raises."""
        cnt = len(hops)
        assert len(bs) == cnt and len(xs) == cnt and len(shifts) == cnt
        if cnt == 0:
            return []
        diags = [None] * cnt if diags is None else list(diags)
        masks = [None] * cnt if masks is None else list(masks)
        assert len(diags) == cnt and len(masks) == cnt
        code, two = xs[0].code, bool(hops[0].twolayer)
        for hop, b, x, dg, mk in zip(hops, bs, xs, diags, masks):
            assert bool(hop.twolayer) == two and x.code == code
            self._pcg_operands(int(np.prod(hop.cshape)), b, x, dg, mk)
        harr = (mpse_heff * cnt)(*[hop.heff for hop in hops])
        ptrs = lambda ts: (C.c_void_p * cnt)(*[None if t is None else t.ptr for t in ts])
        sh = (C.c_double * cnt)(*[float(v) for v in shifts])
        st, it = (C.c_int * cnt)(), (C.c_int * cnt)()
        rel, lv = (C.c_double * cnt)(), (C.c_double * cnt)()
        self._check(self.lib.mpse_pcg_batch(self.ctx, code, cnt, harr, int(two), sh, ptrs(diags), ptrs(masks), ptrs(bs),
                                            ptrs(xs), float(tol), int(max_iter), st, it, rel, lv))
        return [self._pcg_result(st[i], it[i], rel[i], lv[i]) for i in range(cnt)]

    # -- two MPO layers on a two-leg centre: the terms of the finite-temperature correction-vector operator
    def ft_term(self, w1, w2, leg1, leg2, trans1, trans2, shape, L=None, R=None):
        """Descriptor (``mpse_heff_ft``) of one term on a centre / site of ``shape`` (Dl, d_up, d_down, Dr): MPO sites
        ``w1`` (layer 1) and ``w2`` on the legs ``leg1`` / ``leg2``; ``L`` / ``R`` the term's environments (not needed
        for an environment update).  The descriptor keeps no reference: the caller holds the tensors."""
        h = mpse_heff_ft()
        h.Dl, h.d_up, h.d_down, h.Dr = [int(v) for v in shape]
        h.wl1, h.wr1, h.wl2, h.wr2 = w1.shape[0], w1.shape[3], w2.shape[0], w2.shape[3]
        h.leg1, h.leg2, h.trans1, h.trans2 = int(leg1), int(leg2), int(bool(trans1)), int(bool(trans2))
        assert w1.dtype == w2.dtype
        h.W1, h.W2, h.w_dtype = w1.ptr, w2.ptr, w1.code
        if L is not None:
            assert L.shape == (h.Dl, h.wl1, h.wl2, h.Dl), (L.shape, shape)
            h.L, h.l_dtype = L.ptr, L.code
        if R is not None:
            assert R.shape == (h.Dr, h.wr1, h.wr2, h.Dr), (R.shape, shape)
            h.R, h.r_dtype = R.ptr, R.code
        return h

    def heff_apply_ft(self, term, c):
        """``term`` applied to the centre ``c`` (``mpse_heff_apply_ft``)."""
        out = self.empty(c.shape, c.dtype)
        self._check(self.lib.mpse_heff_apply_ft(self.ctx, c.code, C.byref(term), c.ptr, out.ptr))
        return out

    def env_update_ft(self, term, domain, env, x):
        """The environment ``env`` of ``term`` moved over the site ``x`` (bra = conj(x)); ``domain`` "L" or "R"
        (``mpse_env_update_ft``).  Returns the new environment (ket bond, layer 1, layer 2, bra bond)."""
        left = domain == "L"
        oshape = (term.Dr, term.wr1, term.wr2, term.Dr) if left else (term.Dl, term.wl1, term.wl2, term.Dl)
        dt = np.complex128 if (x.is_complex or env.is_complex) else np.float64
        assert x.dtype == dt, "the site must have the working dtype"
        out = self.empty(oshape, dt)
        self._check(self.lib.mpse_env_update_ft(self.ctx, x.code, DOMAIN_L if left else DOMAIN_R, C.byref(term),
                                                env.ptr, env.code, x.ptr, out.ptr))
        return out

    def site_factor_ft(self, term):
        """Per-site factor of the diagonal of ``term`` (``mpse_site_factor_ft``): depends on the two MPO sites only."""
        s = self.empty((term.wl1, term.wl2, term.d_up, term.d_down, term.wr1, term.wr2), np.float64)
        self._check(self.lib.mpse_site_factor_ft(self.ctx, C.byref(term), s.ptr))
        return s

    def diag_ft_sum(self, terms, factors, weights, shift):
        """``shift + sum_t weights[t] * diag(terms[t])`` as a float64 device tensor of the centre's shape."""
        t0 = terms[0]
        diag = self.empty((t0.Dl, t0.d_up, t0.d_down, t0.Dr), np.float64)
        for k, (t, s, w) in enumerate(zip(terms, factors, weights)):
            self._check(self.lib.mpse_diag_ft(self.ctx, C.byref(t), s.ptr, float(w), float(shift), int(k > 0), diag.ptr))
        return diag

    PCG_SUM_STATS = ("solves", "iterations", "term_applies", "host_waits", "diagonals")

    def pcg_sum_stats(self):
        """{name: count} of the summed conjugate-gradient solves (``mpse_pcg_sum_stats``), cumulative."""
        return self._stats_dict(self.lib.mpse_pcg_sum_stats, self.PCG_SUM_STATS)

    def pcg_sum(self, terms, weights, b, x, diag=None, mask=None, shift=0.0, tol=1e-5, max_iter=0, check=True):
        """Solve ``(mask * sum_t weights[t] * terms[t] + shift) x = b`` (``mpse_pcg_sum``); arguments and result as
        ``pcg``, ``terms`` a list of ``ft_term`` descriptors."""
        nt = len(terms)
        arr = (mpse_heff_ft * nt)(*terms)
        w = (C.c_double * nt)(*[float(v) for v in weights])
        self._pcg_operands(x.size, b, x, diag, mask)
        it, rel, lv = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        st = self.lib.mpse_pcg_sum(self.ctx, x.code, nt, arr, w, float(shift), None if diag is None else diag.ptr,
                                   None if mask is None else mask.ptr, b.ptr, x.ptr, float(tol), int(max_iter),
                                   C.byref(it), C.byref(rel), C.byref(lv))
        return self._pcg_result(st, it.value, rel.value, lv.value, check)

    # -- overlap of two chains
    OVERLAP_STATS = ("chain_kernel", "enqueued", "sites")

    def mps_overlap_stats(self):
        """{name: count} of the ``mps_overlap`` calls of this context, cumulative (``mpse_mps_overlap_stats``): chains
        taken by the chain kernel, chains taken by the enqueued products, sites walked."""
        return self._stats_dict(self.lib.mpse_mps_overlap_stats, self.OVERLAP_STATS)

    def mps_overlap(self, bra_sites, ket_sites, conj_bra):
        """<bra|ket> of two chains of device site tensors (D_l, p.., D_r) in one engine call (``mpse_mps_overlap``);
        every leg between the bonds is summed, so MpDm sites pass as they are.  ``conj_bra``: conjugate the bra inside
        the contraction.  Real and complex sites may be mixed.  Returns a complex."""
        n = len(bra_sites)
        if n != len(ket_sites) or n == 0:
            raise ValueError(f"mps_overlap: {n} bra sites, {len(ket_sites)} ket sites")
        dims = (C.c_int64 * (5 * n))()
        for i, (b, k) in enumerate(zip(bra_sites, ket_sites)):
            pb, pk = b.size // (b.shape[0] * b.shape[-1]), k.size // (k.shape[0] * k.shape[-1])
            if pb != pk:
                raise ValueError(f"mps_overlap: site {i} has physical extents {b.shape[1:-1]} and {k.shape[1:-1]}")
            dims[5 * i:5 * i + 5] = [b.shape[0], k.shape[0], pb, b.shape[-1], k.shape[-1]]
        out = (C.c_double * 2)()
        self._check(self.lib.mpse_mps_overlap(
            self.ctx, n, *_site_args(bra_sites), *_site_args(ket_sites), dims, int(bool(conj_bra)), out))
        return complex(out[0], out[1])

    # -- <bra| O |ket> of two chains and an MPO
    SANDWICH_STATS = ("chain_kernel", "enqueued", "sites")

    def mps_sandwich_stats(self):
        """{name: count} of the ``mps_sandwich`` calls of this context, cumulative (``mpse_mps_sandwich_stats``): chains
        taken by the chain kernel, chains taken by the enqueued environment updates, sites walked."""
        return self._stats_dict(self.lib.mpse_mps_sandwich_stats, self.SANDWICH_STATS)

    @staticmethod
    def sandwich_dims(bra_sites, w_sites, ket_sites):
        """The ``dims`` rows (Db_l, Dk_l, wl, d, danc, Db_r, Dk_r, wr) of a chain of site tensors (D_l, d[, danc], D_r)
        and MPO sites (wl, d, d, wr); ValueError when the three do not describe the same sites."""
        n = len(bra_sites)
        if n == 0 or n != len(ket_sites) or n != len(w_sites):
            raise ValueError(f"mps_sandwich: {n} bra sites, {len(w_sites)} MPO sites, {len(ket_sites)} ket sites")
        rows = []
        for i, (b, w, k) in enumerate(zip(bra_sites, w_sites, ket_sites)):
            if b.ndim not in (3, 4) or k.ndim != b.ndim or w.ndim != 4 or tuple(b.shape[1:-1]) != tuple(k.shape[1:-1]) \
                    or w.shape[1] != b.shape[1] or w.shape[2] != b.shape[1]:
                raise ValueError(f"mps_sandwich: site {i} has shapes {b.shape}, {w.shape}, {k.shape}")
            rows.append([b.shape[0], k.shape[0], w.shape[0], b.shape[1], b.shape[2] if b.ndim == 4 else 1, b.shape[-1],
                         k.shape[-1], w.shape[3]])
        return rows

    def mps_sandwich(self, bra_sites, w_sites, ket_sites, conj_bra):
        """<bra| O |ket> of two chains of device site tensors (D_l, d[, danc], D_r) and the device sites (wl, d, d, wr)
        of an MPO in one engine call (``mpse_mps_sandwich``); the first physical leg of an MPO site meets the bra, the
        ancilla leg of density-operator sites is traced.  ``conj_bra``: conjugate the bra inside the contraction.  Real
        and complex tensors may be mixed.  Returns a complex."""
        rows = self.sandwich_dims(bra_sites, w_sites, ket_sites)
        n = len(rows)
        dims = (C.c_int64 * (8 * n))(*[int(x) for r in rows for x in r])
        out = (C.c_double * 2)()
        self._check(self.lib.mpse_mps_sandwich(
            self.ctx, n, *_site_args(bra_sites), *_site_args(ket_sites), *_site_args(w_sites), dims, int(bool(conj_bra)),
            out))
        return complex(out[0], out[1])

    # -- matrix of two-point functions of one-site operators
    CORR_STATS = ("chain_kernel", "enqueued", "sites", "entries")

    def mps_corr_stats(self):
        """{name: count} of the ``mps_corr`` calls of this context, cumulative (``mpse_mps_corr_stats``): calls taken by
        the chain kernels, calls taken by the enqueued products, sites walked, matrix entries produced."""
        return self._stats_dict(self.lib.mpse_mps_corr_stats, self.CORR_STATS)

    @staticmethod
    def corr_dims(sites):
        """The ``dims`` rows (D_l, d, danc, D_r) of a chain of site tensors (D_l, d[, danc], D_r)"""
        rows = []
        for i, t in enumerate(sites):
            if t.ndim not in (3, 4):
                raise ValueError(f"mps_corr: site {i} has shape {t.shape}")
            rows.append([t.shape[0], t.shape[1], t.shape[2] if t.ndim == 4 else 1, t.shape[-1]])
        return rows

    @classmethod
    def _sel_dims(cls, call, sites, sel):
        """(rows, number of sites, selection as ints, dims array) of a chain call with a site selection; ValueError for
        an empty chain or a selection that is not one.  Needs no context."""
        rows = cls.corr_dims(sites)
        n = len(rows)
        if n == 0:
            raise ValueError(f"{call}: no sites")
        sel = check_selection(call, sel, n)
        return rows, n, sel, (C.c_int64 * (4 * n))(*[int(x) for r in rows for x in r])

    def mps_corr(self, sites, sel, x_mats, y_mats, z_mats):
        """C[k, l] = <psi| X_k Y_l |psi> (k < l), C[k, k] = <psi| Z_k |psi> for one-site operators on the sites ``sel``
        (strictly ascending) of a chain of device site tensors (D_l, d[, danc], D_r), in one engine call
        (``mpse_mps_corr``).  ``x_mats`` / ``y_mats`` / ``z_mats``: one (d, d) host matrix per selected site, first
        index on the bra side; the ancilla leg of density-operator sites is traced.  Returns an (nsel, nsel) complex
        array whose lower triangle is zero."""
        rows = self.corr_dims(sites)
        n, nsel = len(rows), len(sel)
        if n == 0 or nsel == 0 or not (len(x_mats) == len(y_mats) == len(z_mats) == nsel):
            raise ValueError(f"mps_corr: {n} sites, {nsel} selected, {len(x_mats)}/{len(y_mats)}/{len(z_mats)} matrices")
        packed = []
        for mats in (x_mats, y_mats, z_mats):
            flat = []
            for k, m in zip(sel, mats):
                m = np.ascontiguousarray(m, dtype=np.complex128)
                d = rows[k][1] if 0 <= int(k) < n else m.shape[0]
                if m.shape != (d, d):
                    raise ValueError(f"mps_corr: a local matrix of site {k} has shape {m.shape}, the site has d = {d}")
                flat.append(m.reshape(-1))
            packed.append(np.ascontiguousarray(np.concatenate(flat)).view(np.float64))
        dims = (C.c_int64 * (4 * n))(*[int(x) for r in rows for x in r])
        out = np.zeros((nsel, nsel), dtype=np.complex128)
        self._check(self.lib.mpse_mps_corr(
            self.ctx, n, *_site_args(sites), dims, nsel, (C.c_int * nsel)(*[int(k) for k in sel]),
            *[p.ctypes.data_as(_dblp) for p in packed], out.ctypes.data_as(_dblp)))
        return out

    # -- one-site reduced density matrices
    RDM1_STATS = ("chain_kernel", "enqueued", "sites", "matrices")

    def mps_rdm1_stats(self):
        """{name: count} of the ``mps_rdm1`` calls of this context, cumulative (``mpse_mps_rdm1_stats``): calls taken by
        the chain kernels, calls taken by the enqueued products, sites walked, matrices produced."""
        return self._stats_dict(self.lib.mpse_mps_rdm1_stats, self.RDM1_STATS)

    def mps_rdm1(self, sites, sel):
        """rho_i[p, p'] = sum conj(A[a,p,g,b]) L_i[a,a'] A[a',p',g,b'] R_i[b,b'] for the sites ``sel`` (strictly
        ascending) of a chain of device site tensors (D_l, d[, danc], D_r), in one engine call (``mpse_mps_rdm1``); L_i
        and R_i are the identity-operator environments of the other sites, the ancilla leg of density-operator sites is
        traced.  Returns a list of (d, d) complex128 arrays, one per selected site."""
        rows, n, sel, dims = self._sel_dims("mps_rdm1", sites, sel)
        sizes = [rows[k][1] ** 2 for k in sel]
        out = np.zeros(sum(sizes), dtype=np.complex128)
        self._check(self.lib.mpse_mps_rdm1(
            self.ctx, n, *_site_args(sites), dims, len(sel), (C.c_int * len(sel))(*sel), out.ctypes.data_as(_dblp)))
        ends = np.cumsum(sizes)
        return [out[e - sz:e].reshape(rows[k][1], rows[k][1]) for k, sz, e in zip(sel, sizes, ends)]

    # -- Schmidt weights of bonds
    BOND_SPECTRA_STATS = ("chain_kernel", "enqueued", "sites", "bonds", "max_sweeps")

    def mps_bond_spectra_stats(self):
        """{name: count} of the ``mps_bond_spectra`` calls of this context, cumulative
        (``mpse_mps_bond_spectra_stats``): calls taken by the chain kernels, calls taken by the enqueued path, sites
        walked, bonds returned, and the largest number of sweeps a Jacobi solve of the chain kernels has taken."""
        return self._stats_dict(self.lib.mpse_mps_bond_spectra_stats, self.BOND_SPECTRA_STATS)

    def mps_bond_spectra(self, sites, sel):
        """The Schmidt weights sigma^2 of the bonds ``sel`` (strictly ascending; bond k lies between the sites k and
        k + 1) of a chain of device site tensors (D_l, d[, danc], D_r), in one engine call
        (``mpse_mps_bond_spectra``): from the two identity-operator environments of each bond, without a canonical
        form; the ancilla leg of density-operator sites is traced.  Returns a list of float64 arrays, one per selected
        bond, each the D_k weights in descending order, not normalised."""
        rows = self.corr_dims(sites)
        n = len(rows)
        if n < 2:
            raise ValueError(f"mps_bond_spectra: a chain of {n} site(s) has no bond")
        sel = check_selection("mps_bond_spectra", sel, n - 1)
        dims = (C.c_int64 * (4 * n))(*[int(x) for r in rows for x in r])
        sizes = [rows[k][3] for k in sel]
        out = np.zeros(sum(sizes), dtype=np.float64)
        self._check(self.lib.mpse_mps_bond_spectra(
            self.ctx, n, *_site_args(sites), dims, len(sel), (C.c_int * len(sel))(*sel), out.ctypes.data_as(_dblp)))
        ends = np.cumsum(sizes)
        return [out[e - sz:e] for sz, e in zip(sizes, ends)]

    # -- expectation values of a list of MPOs
    EXPECT_MANY_STATS = ("chain_kernel", "enqueued", "sites", "entries")

    def mps_expect_many_stats(self):
        """{name: count} of the ``mps_expect_many`` calls of this context, cumulative (``mpse_mps_expect_many_stats``):
        calls taken by the chain kernels, calls taken by the enqueued path, sites walked (the chain's once per call),
        values returned."""
        return self._stats_dict(self.lib.mpse_mps_expect_many_stats, self.EXPECT_MANY_STATS)

    def mps_expect_many(self, sites, operators):
        """<psi| O_m |psi> for a list of MPOs against ONE chain of device site tensors (D_l, d[, danc], D_r), in one
        engine call with one host read (``mpse_mps_expect_many``).  ``operators``: one (first site, [device MPO sites
        (wl, d, d, wr) of the window]) per operator, which is the identity outside its window; the first physical leg
        of an MPO site meets the conjugated tensor, the ancilla leg of density-operator sites is traced.  Real and
        complex tensors may be mixed.  Returns a complex128 array of len(operators) values."""
        rows = self.corr_dims(sites)
        n = len(rows)
        if n == 0 or len(operators) == 0:
            raise ValueError(f"mps_expect_many: {n} sites, {len(operators)} operators")
        wsites, windows = [], []
        for m, (first, ws) in enumerate(operators):
            first, ws = int(first), list(ws)
            if not ws or first < 0 or first + len(ws) > n:
                raise ValueError(f"mps_expect_many: operator {m} has {len(ws)} MPO sites from site {first} of {n}")
            for i, w in enumerate(ws, first):
                if w.ndim != 4 or w.shape[1] != rows[i][1] or w.shape[2] != rows[i][1]:
                    raise ValueError(f"mps_expect_many: operator {m} has shape {w.shape} at site {i}, d = {rows[i][1]}")
            wsites.extend(ws)
            windows.append((first, [(w.shape[0], w.shape[3]) for w in ws]))
        dims = (C.c_int64 * (4 * n))(*[int(x) for r in rows for x in r])
        nop, first, last, wdims = _window_args(windows)
        out = np.zeros(nop, dtype=np.complex128)
        self._check(self.lib.mpse_mps_expect_many(
            self.ctx, n, *_site_args(sites), dims, nop, first, last, *_site_args(wsites), wdims,
            out.ctypes.data_as(_dblp)))
        return out

    # -- tangent-space (TDA) operator
    TDA_STATS = ("handles", "applies", "env_updates", "heff_applies", "qdiag_sites", "davidson")

    def tda_stats(self):
        """{name: count} of the ``mpse_tda_*`` calls of this context, cumulative (``mpse_tda_stats``): handles created,
        applications, the environment updates and effective-Hamiltonian applications they issued, sites through
        k_tda_qdiag, Davidson calls."""
        return self._stats_dict(self.lib.mpse_tda_stats, self.TDA_STATS)

    def tda_operator(self, a, b, u, w):
        """``TdaOperator`` on lists of device tensors (``mpse_tda_create``)"""
        return TdaOperator(self, a, b, u, w)

    # -- two-site reduced density matrices
    RDM2_STATS =("chain_kernel", "enqueued", "sites", "pairs")

    def mps_rdm2_stats(self):
        """{name: count} of the ``mps_rdm2`` calls of this context, cumulative (``mpse_mps_rdm2_stats``): calls taken by
        the chain kernels, calls taken by the enqueued products, sites walked, pairs produced."""
        return self._stats_dict(self.lib.mpse_mps_rdm2_stats, self.RDM2_STATS)

    def mps_rdm2(self, sites, sel):
        """rho_kl[p, p', q, q'] = sum conj(A_k)[.,p,g,.] conj(A_l)[.,q,g',.] A_k[.,p',g,.] A_l[.,q',g',.] for every pair
        k < l of the sites ``sel`` (strictly ascending, at least two) of a chain of device site tensors (D_l, d[, danc],
        D_r), in one engine call (``mpse_mps_rdm2``): identity environments outside the pair, identity transfer matrices
        in between, the ancilla leg of density-operator sites traced.  Returns {(k, l): (d_k, d_k, d_l, d_l) complex128
        array} with site indices as keys."""
        rows, n, sel, dims = self._sel_dims("mps_rdm2", sites, sel)
        if len(sel) < 2:
            raise ValueError(f"mps_rdm2: a pair needs two selected sites, the selection is {sel}")
        pairs = [(k, l) for i, k in enumerate(sel) for l in sel[i + 1:]]
        sizes = [rows[k][1] ** 2 * rows[l][1] ** 2 for k, l in pairs]
        out = np.zeros(sum(sizes), dtype=np.complex128)
        self._check(self.lib.mpse_mps_rdm2(
            self.ctx, n, *_site_args(sites), dims, len(sel), (C.c_int * len(sel))(*sel), out.ctypes.data_as(_dblp)))
        ends = np.cumsum(sizes)
        return {(k, l): out[e - sz:e].reshape(rows[k][1], rows[k][1], rows[l][1], rows[l][1])
                for (k, l), sz, e in zip(pairs, sizes, ends)}

    # -- one-site transition density matrices of two chains
    TRDM1_STATS = ("chain_kernel", "enqueued", "sites", "matrices")

    def mps_trdm1_stats(self):
        """{name: count} of the ``mps_trdm1`` calls of this context, cumulative (``mpse_mps_trdm1_stats``): calls taken
        by the chain kernels, calls taken by the enqueued products, sites walked, matrices produced."""
        return self._stats_dict(self.lib.mpse_mps_trdm1_stats, self.TRDM1_STATS)

    @staticmethod
    def trdm1_dims(bra_sites, ket_sites):
        """The ``dims`` rows (Db_l, Dk_l, d, danc, Db_r, Dk_r) of two chains of site tensors (D_l, d[, danc], D_r);
        ValueError when the two do not describe the same sites.  Needs no context."""
        n = len(bra_sites)
        if n == 0 or n != len(ket_sites):
            raise ValueError(f"mps_trdm1: {n} bra sites, {len(ket_sites)} ket sites")
        rows = []
        for i, (b, k) in enumerate(zip(bra_sites, ket_sites)):
            if b.ndim not in (3, 4) or k.ndim not in (3, 4):
                raise ValueError(f"mps_trdm1: site {i} has shapes {b.shape} and {k.shape}")
            pb = (b.shape[1], b.shape[2] if b.ndim == 4 else 1)
            pk = (k.shape[1], k.shape[2] if k.ndim == 4 else 1)
            if pb != pk:
                raise ValueError(f"mps_trdm1: site {i} has physical and ancilla extents {pb} in the bra, {pk} in the ket")
            rows.append([b.shape[0], k.shape[0], pb[0], pb[1], b.shape[-1], k.shape[-1]])
        return rows

    def mps_trdm1(self, bra_sites, ket_sites, sel, conj_bra):
        """T_i[p, p'] = sum op(B)[b,p,g,b'] L_i[b,k] K[k,p',g,k'] R_i[b',k'] for the sites ``sel`` (strictly ascending)
        of two chains of device site tensors (D_l, d[, danc], D_r), bra and ket, in one engine call
        (``mpse_mps_trdm1``); L_i and R_i are the overlap environments of the other sites, the ancilla leg of
        density-operator sites is traced.  ``conj_bra``: conjugate the bra inside the contraction, as in
        ``mps_overlap``.  Real and complex sites may be mixed.  Returns a list of (d, d) complex128 arrays, one per
        selected site; the trace of each is <bra|ket>."""
        rows = self.trdm1_dims(bra_sites, ket_sites)
        n = len(rows)
        sel = check_selection("mps_trdm1", sel, n)
        dims = (C.c_int64 * (6 * n))(*[int(x) for r in rows for x in r])
        sizes = [rows[k][2] ** 2 for k in sel]
        out = np.zeros(sum(sizes), dtype=np.complex128)
        self._check(self.lib.mpse_mps_trdm1(
            self.ctx, n, *_site_args(bra_sites), *_site_args(ket_sites), dims, int(bool(conj_bra)), len(sel),
            (C.c_int * len(sel))(*sel), out.ctypes.data_as(_dblp)))
        ends = np.cumsum(sizes)
        return [out[e - sz:e].reshape(rows[k][2], rows[k][2]) for k, sz, e in zip(sel, sizes, ends)]

    def block_qr_stats(self):
        """(block QR calls, of which through the Cholesky-QR kernels, of which redone by Householder) of this context."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.mpse_block_qr_stats(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    SVD_STATS = ("decompositions", "column", "gram", "sweeps", "launches", "gram_R", "column_lds")

    def block_svd_stats(self):
        """{name: count}: which block step ran the Jacobi sweeps of the block SVDs of this context, cumulative
        (``mpse_block_svd_stats``; the names follow the order of include/mpsengine.h).  ``gram_R`` (row slabs of the
        most recent Gram decomposition) and ``column_lds`` (bytes of dynamic LDS granted to the column kernel, 0 before
        the first decomposition) are no counts."""
        return self._stats_dict(self.lib.mpse_block_svd_stats, self.SVD_STATS)

    def heff_fused_stats(self):
        """(bond-matrix, two-level-site) effective-Hamiltonian applications that ran as the fused launch."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.mpse_heff_fused_stats(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    GEMM_PATHS = ("launches", "general", "eight_wave", "split_b1", "split_batched", "die_group1", "die_group2", "skew",
                  "tile_order", "masks", "masks_global", "grouped", "grouped_split2")

    def gemm_path_stats(self):
        """{path: count}: how the contraction kernel was launched by this context, cumulative
        (``mpse_gemm_path_stats``; the names follow the order of include/mpsengine.h)."""
        return self._stats_dict(self.lib.mpse_gemm_path_stats, self.GEMM_PATHS)

    PLAN_REUSE = ("keyed", "hits", "mismatches", "evictions", "fused_rebuilds", "order_rebuilds")

    def plan_reuse_stats(self):
        """{name: count} of ``mpse_plan_reuse_stats``: keyed solves (``mpse_solve_slot``), how their slots matched, and
        how often the device rebuilt a kept plan; cumulative, reads the device (synchronous)."""
        return self._stats_dict(self.lib.mpse_plan_reuse_stats, self.PLAN_REUSE)

    def wfold_path_stats(self):
        """{"grouped_mix": grouped launches that formed their beta term in the epilogue from blocks of the MPO site,
        "wmix": launches of the elementwise MPO pass by the contraction plans, "grouped_outmask": grouped launches that
        skipped the result tiles outside the solve's structural mask}, cumulative (counters 13 to 15 of
        ``mpse_gemm_path_stats``)."""
        n = len(self.GEMM_PATHS)
        v = (C.c_int64 * (n + 3))()
        self._check(self.lib.mpse_gemm_path_stats(self.ctx, v, n + 3))
        return {"grouped_mix": int(v[n]), "wmix": int(v[n + 1]), "grouped_outmask": int(v[n + 2])}

    def block_qr_optimistic(self, on):
        """Optimistic mode of the Cholesky-QR path (``mpse_block_qr_optimistic``): breakdowns are not read back per
        decomposition but raise a sticky flag - ``block_qr_check()`` at the end of a step that can be repeated."""
        self._check(self.lib.mpse_block_qr_optimistic(self.ctx, int(bool(on))))

    def block_qr_scheme(self, scheme):
        """0 Householder only, 1 Cholesky-QR for tall blocks (default), 2 Cholesky-QR wherever it applies, -1 the
        environment's setting (``mpse_block_qr_scheme``)."""
        self._check(self.lib.mpse_block_qr_scheme(self.ctx, int(scheme)))

    def block_qr_check(self):
        v = C.c_int(0)
        self._check(self.lib.mpse_block_qr_check(self.ctx, C.byref(v)))
        return bool(v.value)

    def block_qr_pass_stats(self):
        """(blocks factorised by the Cholesky-QR kernels, of them finished after two passes) - synchronous."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.mpse_block_qr_pass_stats(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    QR_PATHS = ("chol_calls", "right_looking", "left_looking", "fallbacks", "blocks", "two_pass", "first_order_pass2",
                "first_order_pass3")

    def block_qr_path_stats(self, since=None):
        """{name: count}: the decisions of the Cholesky-QR path of this context, cumulative (``mpse_block_qr_path_stats``;
        the names follow the order of include/mpsengine.h) - or, with ``since`` (an earlier return value), the counts
        since then.  Synchronous: four of the counters live on the device."""
        now = self._stats_dict(self.lib.mpse_block_qr_path_stats, self.QR_PATHS)
        return now if since is None else {k: now[k] - since[k] for k in self.QR_PATHS}

    def prof_get(self):
        """{variant: dict(ms, flops, bytes, launches)} for the contraction kernel variants."""
        names = {0: "f64xf64", 1: "c128xf64", 2: "f64xc128", 3: "c128xc128", 4: "lanczos_vec", 5: "block_qr", 6: "block_svd",
                 7: "heff_fused"}
        issued_per_mac = {0: 2.0, 1: 4.0, 2: 4.0, 3: 6.0}     # real flops the MFMA units execute per multiply-add
        out = {}
        for v, nm in names.items():
            ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            self._check(self.lib.mpse_prof_get(self.ctx, v, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)))
            out[nm] = dict(ms=ms.value, flops=fl.value, bytes=by.value, launches=n.value)
            if v < 4:
                kt = C.c_int64()
                self._check(self.lib.mpse_prof_get_ktiles(self.ctx, v, C.byref(kt)))
                out[nm]["ktiles"] = kt.value
                out[nm]["issued_flops"] = kt.value * 65536.0 * issued_per_mac[v]
        sw = C.c_int64()
        self._check(self.lib.mpse_prof_get_svd_sweeps(self.ctx, C.byref(sw)))
        out["block_svd"]["sweeps"] = sw.value
        return out

    # -- tensor factories
    def empty(self, shape, dtype=np.float64):
        if isinstance(shape, (int, np.integer)):
            shape = (shape,)
        dtype = np.dtype(dtype)
        dtype_code(dtype)
        n = math.prod(int(x) for x in shape)
        buf = _Buffer(self, n * dtype.itemsize)
        return DeviceTensor(self, buf, 0, shape, dtype)

    def zeros(self, shape, dtype=np.float64):
        t = self.empty(shape, dtype)
        self._check(self.lib.mpse_memset_zero(self.ctx, t.ptr, t.nbytes))
        return t

    def asdevice(self, a, dtype=None):
        if isinstance(a, DeviceTensor):
            if dtype is not None and np.dtype(dtype) != a.dtype:
                if np.dtype(dtype) == np.complex128:
                    return a.to_complex()
                raise TypeError("cannot cast complex device tensor to real")
            return a
        a = np.asarray(a)
        if dtype is None:
            dtype = np.complex128 if np.iscomplexobj(a) else np.float64
        a = np.ascontiguousarray(a, dtype=dtype)
        t = self.empty(a.shape, a.dtype)
        if a.size:
            self._check(self.lib.mpse_memcpy_h2d(self.ctx, t.ptr, a.ctypes.data, a.nbytes))
        return t

    def copy_block(self, dst, dst_row0, dst_col0, src):
        """dst[dst_row0 + r, dst_col0 + c] = src[r, c] for 2-D views of equal dtype (device to device)."""
        assert dst.dtype == src.dtype and dst.ndim == 2 and src.ndim == 2
        es = dst.dtype.itemsize
        rows, cols = src.shape
        assert dst_row0 + rows <= dst.shape[0] and dst_col0 + cols <= dst.shape[1]
        self._check(self.lib.mpse_memcpy_2d(self.ctx, dst.ptr + (dst_row0 * dst.shape[1] + dst_col0) * es,
                                            dst.shape[1] * es, src.ptr, cols * es, cols * es, rows))

    def copy_sub(self, dst, dst_row0, dst_col0, src, src_row0, src_col0, rows, cols):
        """dst[dst_row0 + r, dst_col0 + c] = src[src_row0 + r, src_col0 + c], r < rows, c < cols (2-D, same dtype)."""
        assert dst.dtype == src.dtype and dst.ndim == 2 and src.ndim == 2
        assert dst_row0 + rows <= dst.shape[0] and dst_col0 + cols <= dst.shape[1]
        assert src_row0 + rows <= src.shape[0] and src_col0 + cols <= src.shape[1]
        if rows == 0 or cols == 0:
            return
        es = dst.dtype.itemsize
        self._check(self.lib.mpse_memcpy_2d(self.ctx, dst.ptr + (dst_row0 * dst.shape[1] + dst_col0) * es,
                                            dst.shape[1] * es, src.ptr + (src_row0 * src.shape[1] + src_col0) * es,
                                            src.shape[1] * es, cols * es, rows))

    def ones(self, shape, dtype=np.float64):
        return self.asdevice(np.ones(shape, dtype=dtype))

    # -- general contraction
    def gemm(self, A, B, Cout, m_a, k_a, k_b, n_b, m_c, n_c, conj_a=False, conj_b=False, batch=1,
             sb_a=0, sb_b=0, sb_c=0, alpha=1.0, beta=0.0, skip_zero_tiles=0):
        d = mpse_gemm_desc()
        d.dtype_a, d.dtype_b = A.code, B.code
        d.conj_a, d.conj_b = int(conj_a), int(conj_b)
        d.m_a, d.k_a, d.k_b, d.n_b, d.m_c, d.n_c = m_a, k_a, k_b, n_b, m_c, n_c
        d.batch, d.sb_a, d.sb_b, d.sb_c = int(batch), int(sb_a), int(sb_b), int(sb_c)
        alpha, beta = complex(alpha), complex(beta)
        d.alpha_re, d.alpha_im, d.beta_re, d.beta_im = alpha.real, alpha.imag, beta.real, beta.imag
        d.skip_zero_tiles = int(skip_zero_tiles)
        self._check(self.lib.mpse_gemm(self.ctx, C.byref(d), A.ptr, B.ptr, Cout.ptr))
        return Cout

    def matmul(self, A, B, conj_a=False, conj_b=False, trans_a=False, trans_b=False):
        """(M,K)@(K,N) on 2-D views; trans_* read the operand transposed through strides."""
        a0, a1 = A.shape
        b0, b1 = B.shape
        M, K = (a1, a0) if trans_a else (a0, a1)
        K2, N = (b1, b0) if trans_b else (b0, b1)
        if K != K2:
            raise ValueError(f"matmul shape mismatch {A.shape} {B.shape}")
        dt = np.complex128 if (A.is_complex or B.is_complex) else np.float64
        out = self.empty((M, N), dt)
        m_a, k_a = (idx1(M, 1), idx1(K, a1)) if trans_a else (idx1(M, a1), idx1(K, 1))
        k_b, n_b = (idx1(K, 1), idx1(N, b1)) if trans_b else (idx1(K, b1), idx1(N, 1))
        return self.gemm(A, B, out, m_a, k_a, k_b, n_b, idx1(M, N), idx1(N, 1), conj_a, conj_b)


_ENGINE = None
_LOCK = threading.Lock()
_TLS = threading.local()


def get_engine() -> Engine:
    """Engine of the calling thread (see ``use_engine``), else the process-wide one, created on first use."""
    eng = getattr(_TLS, "engine", None)
    if eng is not None:
        return eng
    global _ENGINE
    with _LOCK:
        if _ENGINE is None:
            _ENGINE = Engine()
        return _ENGINE


def use_engine(eng):
    """Bind ``eng`` (own HIP stream + memory pool) to the calling thread: several independent trajectories can
    then share one GPU from different threads - ctypes releases the GIL inside the engine, and kernels of
    different streams overlap, so one trajectory's latency-bound phases (QR panels, small solves) hide under
    another's contractions.  Pass None to return to the process-wide engine."""
    _TLS.engine = eng
