"""ctypes loader of libgogp_hip.so (the C ABI of include/gogp_hip.h).

There is deliberately NO fallback: if the shared library is missing or a
symbol cannot be bound, importing the binding raises.  Nothing under oracle/
is ever imported from here.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

from .kernel import CDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgogp_hip.so")
HOOKS_PATH = os.path.join(_HERE, "libgogp_testhooks.so")

GOGP_OK, GOGP_EARG, GOGP_ENOTPD, GOGP_EHIP, GOGP_ESTATE, GOGP_ENOMEM, GOGP_ECOND = 0, 1, 2, 3, 4, 5, 6
GOGP_ENOCONV = 7  # gogp_laplace_observe: Newton did not reach the tolerance (the last iterate is stored)
GOGP_LIK_BERNOULLI_LOGIT, GOGP_LIK_POISSON_LOG = 0, 1
GOGP_MAX_CANDIDATES = 16
GOGP_BATCH_MAX_N = 128
GOGP_COV_MAX_M = 4096
GOGP_MULTI_MAX_T = 128
GOGP_BLOCKCV_MAX = 128
GOGP_SPARSE_MAX_M = 4096
GOGP_SPARSE_MULTI_MAX_T = 128

#: every symbol include/gogp_hip.h declares: (name, restype, argtypes)
_dp = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.c_int64
_h = ctypes.c_void_p
_descp = ctypes.POINTER(CDesc)
#: callback types of the sharded evaluation (include/gogp_hip.h)
GOGP_UNIQUE_ID_BYTES = 128


class CXfer(ctypes.Structure):
    _fields_ = [("peer", ctypes.c_int32), ("is_send", ctypes.c_int32), ("buf", ctypes.c_void_p),
                ("bytes", ctypes.c_int64)]


EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(CXfer), ctypes.c_int32)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                ctypes.c_int64)
class CGemmOpts(ctypes.Structure):
    """gogp_test_gemm_opts (include/gogp_testhooks.h): the tile kernel's GemmGrid and the candidate batch."""
    _fields_ = [(n, ctypes.c_int32) for n in ("ktri", "krag0", "new_row0", "kbeg0", "small_below", "prio", "rule",
                                              "tpb_shift", "rblk0", "cblk0", "pr", "Pr", "pc", "Pc", "beta0", "k")]
    _fields_ += [("bstride", ctypes.c_int64)]
    DEFAULTS = dict(ktri=0, krag0=-1, new_row0=-1, kbeg0=0, small_below=384, prio=0, rule=0, tpb_shift=0, rblk0=0,
                    cblk0=0, pr=0, Pr=1, pc=0, Pc=1, beta0=-1, k=1, bstride=0)


class CKParams(ctypes.Structure):
    """gogp_test_kparams (include/gogp_testhooks.h): the kernels' DevParams, stated field by field."""
    _T, _D, _E = 4, 64, 32  # GOGP_MAX_TERMS, GOGP_MAX_NDIM, GOGP_MAX_EVENTS
    _fields_ = [("ndim", ctypes.c_int32), ("nterms", ctypes.c_int32), ("kind", ctypes.c_int32 * _T),
                ("ard", ctypes.c_int32 * _T), ("c", ctypes.c_double * _T), ("w", ctypes.c_double * _T),
                ("inv_len", (ctypes.c_double * _D) * _T), ("noise_var", ctypes.c_double), ("dnoise", ctypes.c_double),
                ("nevents", ctypes.c_int32), ("ev_axis", ctypes.c_int32), ("ev_from", ctypes.c_double * _E),
                ("ev_to", ctypes.c_double * _E), ("ev_disc", ctypes.c_double * _E)]


GOGP_TEST_NACC = 16 + 64  # include/gogp_testhooks.h


class CGemmPlan(ctypes.Structure):
    """gogp_test_gemm_plan_out (include/gogp_testhooks.h)."""
    _fields_ = [("tile", ctypes.c_int32), ("waves", ctypes.c_int32), ("grid_x", ctypes.c_int64),
                ("grid_z", ctypes.c_int64), ("flops", ctypes.c_double), ("tag", ctypes.c_int64)]


GOGP_CG_MAX_RANK, GOGP_CG_MAX_RHS = 1024, 64
GOGP_VECCHIA_MAX_M = 63


class CCgCol(ctypes.Structure):
    """gogp_cg_col (include/gogp_hip.h): one column of a lock-step block of the iterative solver."""
    _fields_ = [("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("rel_residual", ctypes.c_double),
                ("rel_residual_recurrence", ctypes.c_double)]


class CCgInfo(ctypes.Structure):
    """gogp_cg_info (include/gogp_hip.h)."""
    _fields_ = [("rank_used", ctypes.c_int32), ("products", ctypes.c_int32), ("blocks", ctypes.c_int32),
                ("yt_alpha", ctypes.c_double)]


class CCgLmlInfo(ctypes.Structure):
    """gogp_cg_lml_info (include/gogp_hip.h)."""
    _fields_ = [("lml", ctypes.c_double), ("yt_alpha", ctypes.c_double), ("logdet", ctypes.c_double),
                ("logdet_precond", ctypes.c_double), ("logdet_stderr", ctypes.c_double), ("probes", ctypes.c_int32),
                ("blocks", ctypes.c_int32), ("products", ctypes.c_int32), ("lanczos_max", ctypes.c_int32)]


SYMBOLS = [
    ("gogp_desc_check", ctypes.c_int, [_descp]),
    ("gogp_desc_ntheta_noise", ctypes.c_int, [_descp]),
    ("gogp_create", ctypes.c_int, [_descp, ctypes.c_int, ctypes.POINTER(_h)]),
    ("gogp_destroy", None, [_h]),
    ("gogp_last_error", ctypes.c_char_p, [_h]),
    ("gogp_notpd_index", _i64, [_h]),
    ("gogp_graph_info", ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    ("gogp_events_check", ctypes.c_int, [_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("gogp_set_events", ctypes.c_int, [_h, _dp, ctypes.c_int, ctypes.c_int]),
    ("gogp_set_data", ctypes.c_int, [_h, _dp, _dp, _i64]),
    ("gogp_set_data_device", ctypes.c_int, [_h, ctypes.c_void_p, ctypes.c_void_p, _i64]),
    ("gogp_absorb", ctypes.c_int, [_h, _dp, _dp]),
    ("gogp_observe", ctypes.c_int, [_h, _dp, _i64, _dp]),
    ("gogp_observe_full", ctypes.c_int, [_h, _dp, _i64, _dp]),
    ("gogp_lml", ctypes.c_int, [_h, _dp]),
    ("gogp_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_loo", ctypes.c_int, [_h, _dp, _dp, _dp, _dp]),
    ("gogp_loo_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_blockcv_check", ctypes.c_int, [ctypes.POINTER(_i64), _i64, _i64]),
    ("gogp_blockcv_groups", ctypes.c_int, [ctypes.POINTER(_i64), _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("gogp_blockcv", ctypes.c_int, [_h, ctypes.POINTER(_i64), _i64, _dp, _dp, _dp, _dp]),
    ("gogp_blockcv_gradient", ctypes.c_int, [_h, ctypes.POINTER(_i64), _i64, _dp, _i64]),
    ("gogp_laplace_check", ctypes.c_int, [ctypes.c_int32, _dp, _i64]),
    ("gogp_laplace_observe", ctypes.c_int, [_h, ctypes.c_int32, _dp, _i64, _dp]),
    ("gogp_laplace_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_laplace_get_mode", ctypes.c_int, [_h, _dp, _dp, ctypes.POINTER(ctypes.c_int32)]),
    ("gogp_laplace_produce", ctypes.c_int, [_h, _dp, _i64, _dp, _dp, _dp]),
    ("gogp_multi_set_outputs", ctypes.c_int, [_h, _dp, _i64, ctypes.c_int32]),
    ("gogp_multi_lml", ctypes.c_int, [_h, _dp, _dp]),
    ("gogp_multi_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_multi_get_alpha", ctypes.c_int, [_h, _dp]),
    ("gogp_multi_produce", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_sparse_set_data", ctypes.c_int, [_h, _dp, _dp, _i64, _dp, _i64]),
    ("gogp_sparse_observe", ctypes.c_int, [_h, _dp, _i64, _dp]),
    ("gogp_sparse_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_sparse_produce", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_sparse_set_inducing", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_sparse_gradient_inducing", ctypes.c_int, [_h, _dp, _i64, _dp]),
    ("gogp_basis_set", ctypes.c_int, [_h, _dp, _i64, ctypes.c_int32]),
    ("gogp_basis_lml", ctypes.c_int, [_h, _dp]),
    ("gogp_basis_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_basis_get_beta", ctypes.c_int, [_h, _dp, _dp]),
    ("gogp_basis_get_alpha", ctypes.c_int, [_h, _dp]),
    ("gogp_basis_produce", ctypes.c_int, [_h, _dp, _dp, _i64, _dp, _dp]),
    ("gogp_sparse_multi_set_outputs", ctypes.c_int, [_h, _dp, _i64, ctypes.c_int32]),
    ("gogp_sparse_multi_observe", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_sparse_multi_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_sparse_multi_gradient_inducing", ctypes.c_int, [_h, _dp, _i64, _dp]),
    ("gogp_sparse_multi_produce", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_sparse_select_inducing", ctypes.c_int,
     [_h, _dp, _i64, _dp, _i64, _i64, ctypes.c_double, ctypes.POINTER(_i64), _dp, _dp, ctypes.POINTER(_i64), _dp]),
    ("gogp_sparse_select_inducing_resident", ctypes.c_int,
     [_h, _dp, _i64, _i64, ctypes.c_double, ctypes.POINTER(_i64), _dp, _dp, ctypes.POINTER(_i64), _dp]),
    ("gogp_cg_set_data", ctypes.c_int, [_h, _dp, _dp, _dp, _i64]),
    ("gogp_cg_solve", ctypes.c_int,
     [_h, _dp, _i64, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(CCgInfo),
      ctypes.POINTER(CCgCol)]),
    ("gogp_cg_get_alpha", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_cg_solve_columns", ctypes.c_int,
     [_h, _dp, _i64, ctypes.c_double, ctypes.c_int32, _dp, ctypes.POINTER(CCgCol)]),
    ("gogp_cg_produce", ctypes.c_int,
     [_h, _dp, _i64, _dp, _dp, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(CCgCol)]),
    ("gogp_cg_last_info", ctypes.c_int, [_h, ctypes.POINTER(CCgInfo)]),
    ("gogp_cg_lml_gradient", ctypes.c_int,
     [_h, _dp, _i64, _i64, ctypes.c_double, ctypes.c_int32, _dp, _i64, _dp, ctypes.POINTER(CCgLmlInfo),
      ctypes.POINTER(CCgCol)]),
    ("gogp_vecchia_check", ctypes.c_int, [ctypes.POINTER(ctypes.c_int32), _i64, ctypes.c_int32, _i64, ctypes.c_int]),
    ("gogp_vecchia_set_data", ctypes.c_int, [_h, _dp, _dp, _dp, _i64, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    ("gogp_vecchia_observe", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_vecchia_gradient", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_vecchia_produce", ctypes.c_int, [_h, _dp, _i64, ctypes.POINTER(ctypes.c_int32), _dp, _dp]),
    ("gogp_vecchia_neighbours", ctypes.c_int,
     [_h, _dp, _i64, _dp, _i64, _dp, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("gogp_vecchia_set_data_nearest", ctypes.c_int, [_h, _dp, _dp, _dp, _i64, _dp, ctypes.c_int32]),
    ("gogp_vecchia_reneighbour", ctypes.c_int, [_h, _dp]),
    ("gogp_vecchia_get_neighbours", ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int32)]),
    ("gogp_vecchia_produce_nearest", ctypes.c_int, [_h, _dp, _i64, _dp, _dp, _dp, ctypes.POINTER(ctypes.c_int32)]),
    ("gogp_observe_gradient_batch", ctypes.c_int,
     [ctypes.POINTER(_h), ctypes.c_int, _dp, _i64, _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_observe_gradient_candidates", ctypes.c_int,
     [_h, ctypes.c_int, _dp, _i64, _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_batch_set_data", ctypes.c_int,
     [_h, _dp, _dp, _i64, ctypes.c_int32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("gogp_batch_observe_gradient", ctypes.c_int,
     [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), _dp, _i64, _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_batch_produce", ctypes.c_int,
     [_h, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), _dp, _i64, ctypes.POINTER(_i64), _dp, _dp, _dp, _dp,
      ctypes.POINTER(ctypes.c_int)]),
    ("gogp_batch_observe_full_gradient", ctypes.c_int,
     [_h, ctypes.c_int32, _dp, ctypes.POINTER(_i64), _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_batch_produce_full", ctypes.c_int,
     [_h, ctypes.c_int32, _dp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _dp, _dp, _dp, _dp,
      ctypes.POINTER(ctypes.c_int)]),
    ("gogp_produce", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_produce_gradient", ctypes.c_int, [_h, _dp, _i64, _dp, _dp, _dp, _dp]),
    ("gogp_produce_covariance", ctypes.c_int, [_h, _dp, _i64, _dp, _dp]),
    ("gogp_produce_samples", ctypes.c_int, [_h, _dp, _i64, _dp, _i64, ctypes.c_double, _dp, _dp]),
    ("gogp_n", _i64, [_h]),
    ("gogp_get_alpha", ctypes.c_int, [_h, _dp]),
    ("gogp_get_factor", ctypes.c_int, [_h, _dp]),
    ("gogp_get_factor_rows", ctypes.c_int, [_h, ctypes.POINTER(_i64), _i64, _dp]),
    ("gogp_get_factor_diag", ctypes.c_int, [_h, _dp]),
    ("gogp_set_factor", ctypes.c_int, [_h, _dp, _dp, _dp, _dp]),
    ("gogp_append", ctypes.c_int, [_h, _dp, _dp, ctypes.c_int64]),
    ("gogp_append_noisy", ctypes.c_int, [_h, _dp, _dp, _dp, ctypes.c_int64]),
    ("gogp_noise_variances_check", ctypes.c_int, [_dp, _i64]),
    ("gogp_set_noise_variances", ctypes.c_int, [_h, _dp, _i64]),
    ("gogp_get_noise_variances", ctypes.c_int, [_h, _dp]),
    ("gogp_noise_variances_gradient", ctypes.c_int, [_h, _dp]),
    ("gogp_remove", ctypes.c_int, [_h, ctypes.POINTER(_i64), ctypes.c_int64]),
    ("gogp_dist_grid", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("gogp_dist_unique_id", ctypes.c_int, [ctypes.c_void_p]),
    ("gogp_dist_init_rccl", ctypes.c_int,
     [_h, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    ("gogp_dist_init_callbacks", ctypes.c_int,
     [_h, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("gogp_dist_local_bytes", _i64, [_h]),
    ("gogp_dist_comm_ranks", ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_dist_selftest", ctypes.c_int, [_h, ctypes.c_int, _i64]),
    ("gogp_profile_enable", ctypes.c_int, [_h, ctypes.c_int]),
    ("gogp_profile_read", ctypes.c_int, [_h, _dp, ctypes.POINTER(_i64), _dp, _dp]),
    ("gogp_profile_read_launches", ctypes.c_int,
     [_h, _i64, _dp, _dp, _dp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    ("gogp_profile_read_aux", ctypes.c_int, [_h, ctypes.c_int, _dp, ctypes.POINTER(_i64)]),
    ("gogp_set_option", ctypes.c_int, [_h, ctypes.c_char_p, _i64]),
    ("gogp_version", ctypes.c_char_p, []),
]

#: every symbol include/gogp_testhooks.h declares (libgogp_testhooks.so: measurement and
#: diagnostic hooks for tests/, tools/ and bench.py -- not part of the product ABI)
HOOK_SYMBOLS = [
    ("gogp_mfma_f64_peak", ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]),
    ("gogp_mfma_f32_peak", ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]),
    ("gogp_bench_gemm", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, ctypes.c_int, _dp, _dp]),
    ("gogp_test_diag256", ctypes.c_int,
     [ctypes.c_int, _dp, _dp, _dp, ctypes.POINTER(ctypes.c_uint64), _dp]),
    ("gogp_test_dgemm_nt", ctypes.c_int,
     [ctypes.c_int, _i64, _i64, _i64, ctypes.c_double, _dp, _dp, ctypes.c_double, _dp]),
    ("gogp_test_valu_cost", ctypes.c_int, [ctypes.c_int, _dp]),
    ("gogp_test_panel128", ctypes.c_int,
     [ctypes.c_int, _dp, _dp, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), _dp]),
    ("gogp_test_panel128_slabs", ctypes.c_int, [ctypes.c_int, _dp, _dp, _i64, ctypes.c_int, ctypes.c_int, _dp]),
    ("gogp_test_gemm_nt", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, ctypes.c_double, ctypes.c_double]
     + [ctypes.c_void_p, _i64, _i64, _i64] * 3 + [ctypes.POINTER(CGemmOpts)]),
    ("gogp_test_gemm_plan", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, ctypes.POINTER(CGemmOpts),
      ctypes.POINTER(CGemmPlan)]),
    ("gogp_test_diag_syrk", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _i64, _i64, _i64, _i64, _i64, _dp, _i64, ctypes.c_int]),
    ("gogp_test_diag256_product", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, _dp, _i64, _dp, _i64, _dp, _i64, _i64, ctypes.POINTER(ctypes.c_longlong)]),
    # the kernels that consume the factor (tests/test_substitution_kernels.py)
    ("gogp_test_trsm_small_workspace", _i64, [_i64]),
    ("gogp_test_trsm_small", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, _i64, ctypes.c_void_p, _i64, _i64, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64,
      ctypes.c_int, ctypes.c_int, _dp, _i64, ctypes.c_void_p, _i64, ctypes.POINTER(ctypes.c_int),
      ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_uint)]),
    ("gogp_test_trsv_steps", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, ctypes.c_void_p, _i64, _i64, ctypes.c_void_p, ctypes.c_int,
      ctypes.c_int, ctypes.c_int, _i64, _dp, _i64, _dp, _i64]),
    ("gogp_test_alpha_from_y", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, _i64, ctypes.c_void_p, _i64, _i64, _dp, _i64, _dp, _i64]),
    ("gogp_test_rownorm_dot", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _i64, _i64, _i64, _i64, _dp, _i64, _dp, _i64, _dp, _i64]),
    ("gogp_test_tinv", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64, ctypes.c_int,
      ctypes.c_void_p]),
    ("gogp_test_blockmm", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _i64] + [ctypes.POINTER(_i64)] * 6
     + [ctypes.POINTER(ctypes.c_int), ctypes.c_double, ctypes.c_int, _i64]),
    # the kernels that turn K^-1 into the gradient (tests/test_grad_kernels.py)
    ("gogp_test_grad_blocks", ctypes.c_int, [_i64, _i64, _i64, ctypes.c_int]),
    ("gogp_test_grad_reduce", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.POINTER(CKParams)] + [ctypes.c_int] * 4
     + [_dp, _i64, _dp, _i64, ctypes.c_void_p, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, _i64, _dp, _i64, _dp]),
    ("gogp_test_grad_reduce_local", ctypes.c_int,
     [ctypes.c_int, ctypes.c_int, ctypes.POINTER(CKParams)] + [ctypes.c_int] * 4
     + [_dp, _i64, _dp, _i64, ctypes.c_void_p, _i64, _i64, _i64, _i64, _i64, _i64] + [ctypes.c_int] * 7
     + [_i64, _dp, _i64, _dp]),
    ("gogp_test_xgrad", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), ctypes.c_int, _dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64, _dp,
      _i64]),
    # the kernels of Append, Remove, ProduceGradient's product and ProduceCovariance (tests/test_update_kernels.py)
    ("gogp_test_append_gram", ctypes.c_int,
     [ctypes.c_int] + [ctypes.c_void_p, _i64, ctypes.c_int, ctypes.c_int, _i64] * 2
     + [ctypes.c_int, ctypes.c_int, _i64, _i64, _dp, _i64, _dp, _i64, _dp, _i64, _i64]),
    ("gogp_test_append_commit", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), ctypes.c_int, _dp, _i64, _dp, _i64, ctypes.c_int, _i64, _dp, _i64,
      ctypes.c_int, _dp, _i64, _i64, _dp, _i64, ctypes.POINTER(ctypes.c_longlong)]),
    ("gogp_test_nv_append_commit", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), ctypes.c_int, _dp, _i64, _dp, _i64, _dp, _i64, ctypes.c_int, _i64, _dp, _i64,
      ctypes.c_int, _dp, _i64, _i64, _dp, _i64, ctypes.POINTER(ctypes.c_longlong)]),
    ("gogp_test_remove_gather", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, ctypes.POINTER(ctypes.c_int), _i64, _i64, _dp, _i64, _i64]),
    ("gogp_test_remove_w", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, ctypes.POINTER(ctypes.c_int), _i64, ctypes.POINTER(ctypes.c_int), _i64, ctypes.c_int,
      ctypes.c_int, _i64, _i64, _i64, _dp, _i64]),
    ("gogp_test_remove_block", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, ctypes.c_int, ctypes.c_int, _dp, _i64, _dp, _i64, ctypes.c_int, _i64, _i64, _i64]),
    ("gogp_test_bwd_panel", ctypes.c_int,
     [ctypes.c_int, _i64] + [_dp, _i64, _i64, _i64] * 3 + [_i64, _i64, ctypes.c_int, ctypes.c_int]),
    ("gogp_test_pcov_slabs", ctypes.c_int, [_i64, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_test_pcov", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), ctypes.c_int, _dp, _i64, _i64, _dp, _i64, _i64, _i64, ctypes.c_int, _dp, _i64,
      ctypes.c_double, _dp, _i64, _i64, _i64]),
    ("gogp_test_multi_weight", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, ctypes.c_int, _dp, _i64, _i64, _i64, _i64, _dp, _i64]),
    ("gogp_bench_sparse_syrk", ctypes.c_int, [ctypes.c_int, _i64, _i64, ctypes.c_int, _dp, _dp]),
    ("gogp_bench_sparse_xty", ctypes.c_int, [ctypes.c_int, _i64, _i64, _i64, ctypes.c_int, _dp, _dp]),
    ("gogp_test_sparse_syrk", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, _i64, _i64, _i64, _dp, _i64, _dp, _i64, _i64, _dp, _i64]),
    ("gogp_test_sparse_grad", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), _dp, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _dp, _i64,
      ctypes.c_double, ctypes.c_int, _dp]),
    ("gogp_test_sparse_ugrad", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), _dp, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _dp, _i64,
      ctypes.c_double, ctypes.c_int, _dp, _i64]),
    ("gogp_test_sparse_ugrad_slabs", ctypes.c_int, [_i64, _i64, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_test_sparse_ugrad_slabs_bound", ctypes.c_int, [_i64, _i64]),
    ("gogp_test_sparse_xty", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _dp, _i64, _i64]),
    ("gogp_test_sparse_xty_slabs", ctypes.c_int, [_i64, _i64, _i64, ctypes.POINTER(ctypes.c_int64)]),
    ("gogp_test_sparse_xty_slabs_bound", ctypes.c_int, [_i64, _i64, _i64]),
    # greedy selection of inducing points (tests/test_select_inducing_kernels.py)
    ("gogp_test_select_step", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), _dp, _i64, _i64, _dp, _i64, _i64, _i64, ctypes.c_double, _dp, _i64,
      ctypes.POINTER(ctypes.c_ubyte), _i64, _dp, ctypes.POINTER(_i64), _i64, ctypes.c_int, _dp, ctypes.POINTER(_i64), _i64,
      ctypes.POINTER(_i64), _dp]),
    ("gogp_test_select_run", ctypes.c_int,
     [ctypes.c_int, ctypes.POINTER(CKParams), _dp, _i64, _i64, _i64, ctypes.c_double, ctypes.c_int, _dp, _i64,
      ctypes.POINTER(_i64), _dp, _dp, _i64, _dp, _i64, _dp, _i64, ctypes.POINTER(_i64), _dp]),
    # the two kernels of leave-block-out cross-validation (tests/test_blockcv_kernels.py)
    ("gogp_test_blockcv_groups", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, _dp, _i64, _dp, _i64, _i64, ctypes.POINTER(_i64), _i64] + [_dp, _i64] * 6
     + [ctypes.POINTER(_i64), _i64]),
    ("gogp_test_blockcv_apply", ctypes.c_int,
     [ctypes.c_int, _dp, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), _i64, _dp, _i64]),
    # per-rank replay of the sharded sweep (tools/sharded_replay.py): a transport that reads recorded panels
    ("gogp_test_dist_init_replay", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4),
]

#: the hooks of the small finishing kernels of leave-one-out, multi-output and sparse (tests/test_finish_kernels.py), as
#: gp.finish_check reads them: name -> arguments after `device`, in order, each "name:kind" with kind a (array read, followed
#: by its length), o (in / out array, followed by its length), l (int64), i (int) or d (double)
_FINISH_SPEC = {
    "loo_stats": "Kinv:a ld:l alpha:a y:a n:l npad:l mu:o sigma:o logp:o v:o sc:o part:o",
    "loo_scale_symv": "Kinv:a ld:l n:l npad:l sc:a v:a B:o ldb:l upart:o u:o",
    "loo_rank2": "G:o ld:l n:l npad:l u:a alpha:a",
    "multi_dots": "Yt:a At:a ld:l n:l T:i dots:o",
    "sparse_finish_b": "Bacc:a Mp:l inv_s2:d B:o",
    "sparse_copy_upper": "src:a Mp:l dst:o",
    "sparse_weights": "B:a Binv:a g:a Mp:l s4:d T:o S:o",
    "sparse_multi_weights": "B:a Binv:a GG:a Mp:l T:i s4:d Tm:o S:o",
    "sparse_scalars": "C:a B:a Binv:a r:a g:a M:l Mp:l out:o",
    "sparse_sumsq": "y:a n:l out:o",
    "sparse_predict": "A:a V:a ld:l ncols:l m:l prior:a q:a dot:a inv_s2:d mu:o sigma:o",
    "sparse_multi_sigma": "A:a V:a ld:l ncols:l m:l prior:a q:a sigma:o",
    "sparse_multi_dots": "Rt:a Gt:a ld:l M:l T:i tstride:i out:o",
    "sparse_multi_sumsq": "Y:a ldy:l n:l T:i out:o",
    "sparse_multi_pad": "Y:a ldy:l rows:l T:l kp:l rpad:l Yp:o ldp:l",
}
FINISH_HOOKS = {k: [tuple(t.split(":")) for t in v.split()] for k, v in _FINISH_SPEC.items()}
_FINISH_CTYPES = {"a": [_dp, _i64], "o": [_dp, _i64], "l": [_i64], "i": [ctypes.c_int], "d": [ctypes.c_double]}
HOOK_SYMBOLS += [("gogp_test_" + k, ctypes.c_int, [ctypes.c_int] + [t for _, kind in spec for t in _FINISH_CTYPES[kind]])
                 for k, spec in FINISH_HOOKS.items()]


#: the hooks of the kernels of the Laplace approximation (tests/test_laplace_kernels.py), as gp.laplace_kernel_check reads
#: them: the notation of _FINISH_SPEC
_LAPLACE_SPEC = {
    "lap_site": "lik:i f:a y:a a:a n:l npad:l g:o W:o sw:o b:o rho:o part:o out:o",
    "lap_scale_gram": "A:o ld:l n:l npad:l sw:a wcols:l",
    "lap_step": "b:a sw:a beta:a n:l npad:l rhs:o a1:o",
    "lap_interp": "a:a a1:a f:a f1:a t:d n:l npad:l at:o ft:o",
    "lap_weight_vectors": "Binv:a ld:l rho:a n:l npad:l sv:o",
    "lap_symv_u": "Binv:a ld:l n:l npad:l v:a sv:a sw:a upart:o u:o",
    "lap_weight": "G:o ld:l n:l npad:l sw:a u:a a:a",
    "lap_colscale": "KsT:o ld:l rows:l npad:l sw:a",
    "lap_mean": "lik:i mu:a sigma:a m:l mean:o",
}
LAPLACE_HOOKS = {k: [tuple(t.split(":")) for t in v.split()] for k, v in _LAPLACE_SPEC.items()}
HOOK_SYMBOLS += [("gogp_test_" + k, ctypes.c_int, [ctypes.c_int] + [t for _, kind in spec for t in _FINISH_CTYPES[kind]])
                 for k, spec in LAPLACE_HOOKS.items()]


#: the hooks of the kernels of the explicit basis functions (tests/test_basis_kernels.py), as gp.basis_kernel_check reads
#: them: the notation of _FINISH_SPEC
_BASIS_SPEC = {
    "basis_symm": "Kinv:a ldk:l n:l npad:l Ht:a ld:l p:i part:o Wt:o",
    "basis_gram": "Ht:a Wt:a ld:l alpha:a n:l p:i part:o Ag:o",
    "basis_finish": "Ag:a p:i LA:o Ainv:o beta:o scal:o info:o",
    "basis_cols": "Wt:a ld:l n:l p:i LA:a beta:a alpha:a Ct:o",
    "basis_predict": "Hz:a KW:a ldkw:l m:l p:i beta:a Ainv:a mu0:a prior:a q:a mu:o sigma:o",
}
BASIS_HOOKS = {k: [tuple(t.split(":")) for t in v.split()] for k, v in _BASIS_SPEC.items()}
HOOK_SYMBOLS += [("gogp_test_" + k, ctypes.c_int, [ctypes.c_int] + [t for _, kind in spec for t in _FINISH_CTYPES[kind]])
                 for k, spec in BASIS_HOOKS.items()]
HOOK_SYMBOLS += [("gogp_test_basis_symm_slabs", ctypes.c_int, [_i64]), ("gogp_test_basis_gram_slabs", ctypes.c_int, [_i64])]


#: the hooks of the kernels of the per-observation noise variances (tests/test_noise_variances_kernels.py), as
#: gp.noise_variances_kernel_check reads them: the notation of _FINISH_SPEC (the append fold goes through
#: gogp_test_nv_append_commit above: gp.nv_append_commit_check)
_NOISEVAR_SPEC = {
    "nv_diag_add": "A:o ld:l n:l npad:l v:a wcols:l",
    "nv_gradient": "Kinv:a ld:l alpha:a n:l npad:l dv:o",
}
NOISEVAR_HOOKS = {k: [tuple(t.split(":")) for t in v.split()] for k, v in _NOISEVAR_SPEC.items()}
HOOK_SYMBOLS += [("gogp_test_" + k, ctypes.c_int, [ctypes.c_int] + [t for _, kind in spec for t in _FINISH_CTYPES[kind]])
                 for k, spec in NOISEVAR_HOOKS.items()]


#: the hooks of the kernels of the sharded path (dist2d.hip and its helpers in solve.hip) and of the rest of solve.hip
#: (tests/test_shard_kernels.py), as gp.shard_kernel_check reads them: the notation of _FINISH_SPEC and, beyond it, A / O: an
#: array (read, in / out) of float64 or float32 as the argument `precision` says (P: as `precision2` says, in / out), f: a
#: float32 array read, and n / r / B: a float64 / int64 / `precision`-typed array read that may be None (NULL, length 0)
_MAP = "nb_shift:i Pr:i Pc:i pr:i pc:i"
_SHARD_SPEC = {
    "gather_rows": "y:a rows:l %s yloc:o" % _MAP,
    "gather_x": "X:a a:a D:i n:l rows:l %s Xloc:o aloc:o" % _MAP,
    "scatter_tile": "precision:i src:A nb:i n:l row0:l col0:l diag:i r0:l dst:o",
    "gather_rows_of_l": "precision:i Lch:A mloc:i nloc:i %s rows:r n:l diag_only:i out:o" % _MAP,
    "scatter_stage": "precision:i stage:a lds:l Lch:O nloc:i mloc:i bi:i nb:i",
    "transpose_rect": "precision:i src:A lds:l dst:O ldd:l rows:l cols:i",
    "transpose_sq": "precision:i src:A lds:l dst:O ldd:l n:i",
    "copy_block": "dst:o src:a ld:l nb:i rows:l",
    "residual_block": "precision:i W:O Ks:A U:a ld:l recv:n nrecv:i nb:i rows:l",
    "pack_blocks": "dst:o src:a nblk:i blk:l first:i stride:i",
    "convert_block": "precision:i precision2:i src:A lds:l dst:P ldd:l rows:i cols:i",
    "chunk_tdot": "precision:i chunk:A rows:l nb:i v:a part:o out:o",
    "chunk_alpha": "precision:i Ych:A mloc:i nloc:i %s z:a out:o" % _MAP,
    "chunk_sumsq": "precision:i Ych:A mloc:i nloc:i %s n:l part:o out:o" % _MAP,
    "lml_scalars": "precision:i L:A ld:l z:a y:a alpha:n n:l k:i bstride:l scalars:o",
    "alpha_from_y_batched": "Y:a ld:l z:a npad:l k:i bstride:l alpha:o",
    "trace_from_y": "Y:f ld:l n:l npad:l alpha:a part:o out:o",
    "zero_upper_blocks": "precision:i R:O ld:l npad:l k:i bstride:l",
    "ydiag": "precision:i Dinv:A Y:O ld:l k:i bstride:l",
    "zero_block": "precision:i B:O ld:l rows:l cols:l k:i bstride:l",
    "extract_lower": "precision:i L:A ld:l n:l out:o",
    "pack_lower": "precision:i src:a n:l npad:l L:O ld:l",
    "sigma": "prior:a q:n m:l sigma:o",
    "logdet_block": "L:a ld:l row0:l n:l nb:i acc:o",
    "dot": "a:a b:a n:l out:o",
    "sumsq_info": "z:a n:l info:r out:o",
    "vector_op": "op:i precision:i a:O b:B count:l f:d",
}
SHARD_HOOKS = {k: [tuple(t.split(":")) for t in v.split()] for k, v in _SHARD_SPEC.items()}
#: the ops of gogp_test_vector_op
VECTOR_OPS = {"fill": 0, "axpy": 1, "add_vec": 2, "scale": 3, "residual_from": 4, "add_inplace": 5, "info_to_double": 6}
_SHARD_CTYPES = dict(_FINISH_CTYPES, **{k: [ctypes.c_void_p, _i64] for k in "AOPBfrn"})
HOOK_SYMBOLS += [("gogp_test_" + k, ctypes.c_int, [ctypes.c_int] + [t for _, kind in spec for t in _SHARD_CTYPES[kind]])
                 for k, spec in SHARD_HOOKS.items()]
HOOK_SYMBOLS += [("gogp_test_chunk_tdot_scratch", _i64, [_i64, ctypes.c_int])]

#: the hooks of the kernels of gram.hip and of pgrad.hip's forecast derivatives (tests/test_gram_kernels.py; gp.gram_*_check,
#: gp.cross_check, gp.prior_check, gp.kmatvec_check, gp.pgrad_check)
_kpp, _vp, _ci = ctypes.POINTER(CKParams), ctypes.c_void_p, ctypes.c_int
HOOK_SYMBOLS += [
    ("gogp_test_gram_split", _ci, [_ci, _ci, _kpp, _ci, _dp, _i64, _i64, _i64, _i64, _ci, _i64, _vp, _i64, _i64]),
    ("gogp_test_gram_local", _ci, [_ci, _ci, _kpp, _ci, _dp, _i64, _i64, _i64, _i64, _i64] + [_ci] * 5 + [_vp, _i64, _i64]),
    ("gogp_test_cross", _ci, [_ci, _ci, _kpp, _ci, _dp, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _vp, _i64, _i64]),
    ("gogp_test_prior", _ci, [_ci, _kpp, _dp, _i64, _i64, _dp, _i64]),
    ("gogp_test_kmatvec", _ci,
     [_ci, _kpp, _ci, _ci, _dp, _i64, _i64, _i64, _dp, _i64, _dp, _i64, _ci, _ci, _ci, _dp, _i64, _dp, _i64]),
    ("gogp_test_pgrad_slabs", _ci, [_i64, _i64, ctypes.POINTER(ctypes.c_int)]),
    ("gogp_test_pgrad", _ci, [_ci, _kpp, _ci, _dp, _i64, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _dp, _i64, _i64, _dp, _i64]
     + [_dp, _i64] * 3),
]

#: the hooks of the kernels of cg.hip (tests/test_cg_kernels.py; gp.kmm_check, gp.cg_*_check)
_i32p = ctypes.POINTER(ctypes.c_int32)
HOOK_SYMBOLS += [
    ("gogp_test_kmm_slabs", _ci, [_i64, _i64]),
    ("gogp_test_cg_dot_blocks", _ci, [_i64]),
    ("gogp_test_kmm", _ci, [_ci, _kpp, _dp, _i64, _i64, _dp, _i64, _i64, _dp, _i64, _i64, _ci, _dp, _i64, _ci, _ci, _dp, _i64,
                            _dp, _i64, _i64]),
    ("gogp_test_cg_dots", _ci, [_ci, _dp, _i64, _dp, _i64, _i64, _i64, _ci, _ci, _ci, ctypes.c_double, _dp, _i64, _dp, _i64,
                                _dp, _i64, _i32p, _i64]),
    ("gogp_test_cg_update_xr", _ci, [_ci] + [_dp, _i64] * 4 + [_i64, _i64, _ci, _dp, _i64, _i32p, _i64]),
    ("gogp_test_cg_update_p", _ci, [_ci] + [_dp, _i64] * 2 + [_i64, _i64, _ci, _dp, _i64, _i32p, _i64]),
    ("gogp_test_cg_scale", _ci, [_ci] + [_dp, _i64] * 3 + [_i64, _i64, _ci, _dp, _i64]),
    ("gogp_test_cg_status", _ci, [_ci, _ci, _i32p, _i64]),
    ("gogp_test_cg_grad", _ci, [_ci, _kpp, _dp, _i64, _i64, _dp, _i64, _dp, _i64, _i64, _ci, ctypes.c_double, _ci, _dp]),
    ("gogp_test_cg_probes", _ci, [_ci, _dp, _i64, _i64, _i64, _ci, _dp, _i64, _dp, _i64, _i64, _i64, _ci, _dp, _i64]),
    ("gogp_test_cg_quadrature", _ci, [_dp, _dp, _i64, ctypes.c_double, _dp]),
    ("gogp_test_cg_precond", _ci, [_ci, _dp, _i64, _i64, _i64, _ci, _dp, _i64, _dp, _i64, _dp, _i64, _i64, _ci, _dp, _i64,
                                   _dp, _i64]),
]

#: the hook of the kernel of vecchia.hip (tests/test_vecchia_kernel.py; gp.vecchia_check)
HOOK_SYMBOLS += [
    ("gogp_test_vecchia_blocks", _ci, [_i64, _ci]),
    ("gogp_test_vecchia", _ci, [_ci, _kpp, _ci, _ci, _dp, _i64, _dp, _i64, _dp, _i64, _i64, _dp, _i64, _i64, _i32p, _i64, _ci,
                                _dp, _i64, _dp, _i64, _dp, _i64, _dp, ctypes.POINTER(_i64), _ci]),
]

#: the hooks of the search of vecchia_knn.hip (tests/test_vecchia_knn_kernel.py; gp.vecchia_knn_check, gp.vecchia_knn_plan)
HOOK_SYMBOLS += [
    ("gogp_test_vecchia_knn", _ci, [_ci, _dp, _i64, _i64, _ci, _dp, _i64, _i64, _dp, _ci, _ci, _ci, _i32p, _i64, _dp, _i64,
                                    _dp, _i64]),
    ("gogp_test_vecchia_knn_plan", _ci, [_i64, _i64, _ci, ctypes.POINTER(_i64)]),
]


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into gogp_amd/libgogp_hip.so
    (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-j8", "-s"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("build did not produce %s" % LIB_PATH)
    return LIB_PATH


_lib = None
_hooks = None


def hooks() -> ctypes.CDLL:
    """The measurement-hook library (include/gogp_testhooks.h)."""
    global _hooks
    if _hooks is None:
        lib()  # the hook library links the product library
        if not os.path.exists(HOOKS_PATH):
            raise ImportError("%s is missing: run __graft_entry__.build()" % HOOKS_PATH)
        L = ctypes.CDLL(HOOKS_PATH)
        for name, restype, argtypes in HOOK_SYMBOLS:
            f = getattr(L, name)
            f.restype = restype
            f.argtypes = argtypes
        _hooks = L
    return _hooks


def lib() -> ctypes.CDLL:
    """The bound library.  Raises (never falls back) if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(gogp_amd has no CPU fallback)" % LIB_PATH)
        # PyTorch's wheel bundles its own copies of the HIP runtime and RCCL whose NEEDED names
        # lack the version suffix: if it is imported AFTER this library, the loader does not
        # match them with the already-loaded /opt/rocm copies and the process ends up with two
        # HIP runtimes (observed: heap corruption at exit).  Where torch exists, load it first;
        # this library then binds to the copies torch loaded (same SONAMEs).  Hosts without
        # torch (the C++ / Go bindings) are not affected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # RTLD_GLOBAL: libgogp_testhooks.so resolves the internal launchers against it
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, restype, argtypes in SYMBOLS:
            f = getattr(L, name)  # AttributeError if the symbol is not exported
            f.restype = restype
            f.argtypes = argtypes
        _lib = L
    return _lib
