"""CPU side of tests/test_tile_kernels.py: the tile-kernel, diagonal-update and diagonal-block hooks refuse arguments
the kernels cannot honour with GOGP_EARG BEFORE touching the device (so these pass on a machine without a GPU), and the
Python wrappers refuse arrays that do not cover the launch before calling the hook at all."""
import ctypes

import numpy as np
import pytest

from gogp_amd import _lib

T = 128


@pytest.fixture(scope="module")
def hk():
    _lib.build()
    return _lib.hooks()


def gemm(hk, prec=64, mode=0, mt=2, nt=2, K=32, alpha=-1.0, beta=1.0, lda=None, ldb=None, ldc=None, a_off=0, b_off=0,
         c_off=0, a_len=None, b_len=None, c_len=None, **opts):
    dt = np.float64 if prec == 64 else np.float32
    lda, ldb, ldc = lda or K, ldb or K, ldc or nt * T
    nb = mt if mode in (1, 2) else nt
    o = dict(_lib.CGemmOpts.DEFAULTS, **opts)
    k, bs = o["k"], o["bstride"]
    a_len = a_len or a_off + (k - 1) * bs + (mt * T - 1) * lda + K
    b_len = b_len or b_off + (k - 1) * bs + (nb * T - 1) * ldb + K
    c_len = c_len or c_off + (k - 1) * bs + (mt * T - 1) * ldc + nt * T
    A, B, C = np.zeros(a_len, dt), np.zeros(b_len, dt), np.zeros(c_len, dt)
    return hk.gogp_test_gemm_nt(-1, prec, mode, mt, nt, K, alpha, beta, A.ctypes.data, a_len, a_off, lda,
                                B.ctypes.data, b_len, b_off, ldb, C.ctypes.data, c_len, c_off, ldc,
                                ctypes.byref(_lib.CGemmOpts(**o)))


REFUSED = [
    dict(prec=16),
    dict(mode=4),
    dict(K=24),                                   # fp64 K-step is 16
    dict(prec=32, K=48),                          # fp32 K-step is 32: a multiple of 16 is not enough
    dict(K=0),
    dict(lda=33),                                 # fp64 rows not 16-byte aligned
    dict(prec=32, lda=34),                        # fp32 rows not 16-byte aligned
    dict(ldc=2 * T + 1),
    dict(a_off=1),
    dict(prec=32, c_off=2),
    dict(lda=16),                                 # leading dimension below the operand
    dict(ldc=T),
    dict(mode=1, mt=2, nt=3),                     # LOWER needs a square tile grid
    dict(mode=2, mt=3, nt=2),                     # so does LAUUM
    dict(alpha=0.0),                              # accumulators start at (beta / alpha) C
    dict(prec=32, alpha=1e-50),                   # zero in fp32
    dict(prec=32, k=2, bstride=1 << 20),          # the fp32 kernel has no candidate batch
    dict(prec=32, mode=2, kbeg0=32),              # nor the two-launch LAUUM
    dict(mode=2, kbeg0=8),                        # kbeg0 not on a K-step
    dict(mode=0, kbeg0=16),                       # kbeg0 is LAUUM's
    dict(mode=0, new_row0=1),                     # new_row0 is LOWER's
    dict(mode=1, ktri=1),                         # ktri is RECT's
    dict(mode=2, krag0=0),                        # krag0 is RECT / LOWER's
    dict(krag0=0, K=128),                         # tile row 1 would start its loads at k = K
    dict(rule=3),
    dict(mode=1, rule=1),
    dict(rule=1, Pr=2, pr=2),
    dict(k=2, bstride=0),
    dict(k=2, bstride=3),                         # slots not 16-byte aligned
    dict(a_len=100),                              # arrays that do not cover the launch
    dict(c_len=2 * T * 2 * T - 1),
    dict(k=3, bstride=1 << 16, b_len=(2 * T - 1) * 32 + 32 + (1 << 16)),  # the third slot of B is missing
]


@pytest.mark.parametrize("bad", REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in REFUSED])
def test_gemm_hook_refuses(hk, bad):
    assert gemm(hk, **bad) == _lib.GOGP_EARG


def test_gemm_hook_accepts_the_valid_neighbours(hk):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in (dict(), dict(prec=32, K=64), dict(mode=1, mt=3, nt=3), dict(mode=2, kbeg0=16), dict(krag0=0, K=256),
               dict(k=2, bstride=1 << 16), dict(rule=2, Pr=2, pr=1, beta0=1, tpb_shift=1)):
        assert gemm(hk, **ok) in (_lib.GOGP_OK, _lib.GOGP_EHIP), ok


def gemm_plan(hk, prec=64, mode=0, mt=2, nt=2, K=32, out=True, **opts):
    res = _lib.CGemmPlan()
    return hk.gogp_test_gemm_plan(prec, mode, mt, nt, K, ctypes.byref(_lib.CGemmOpts(**dict(_lib.CGemmOpts.DEFAULTS, **opts))),
                                  ctypes.byref(res) if out else None)


PLAN_REFUSED = [dict(prec=16), dict(prec=0), dict(mode=4), dict(mode=-1), dict(mt=0), dict(nt=-1), dict(K=0), dict(K=24),
                dict(prec=32, K=48), dict(mode=1, mt=2, nt=3), dict(prec=32, k=2, bstride=1 << 20),
                dict(prec=32, mode=2, kbeg0=32), dict(mode=0, kbeg0=16), dict(mode=1, ktri=1), dict(rule=3),
                dict(k=2, bstride=0), dict(out=False)]


@pytest.mark.parametrize("bad", PLAN_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in PLAN_REFUSED])
def test_gemm_plan_hook_refuses(hk, bad):
    assert gemm_plan(hk, **bad) == _lib.GOGP_EARG


def test_gemm_plan_hook_accepts_the_valid_neighbours(hk):
    for ok in (dict(), dict(prec=32, K=64), dict(mode=3), dict(mode=1, mt=3, nt=3), dict(mode=2, kbeg0=16),
               dict(k=2, bstride=1 << 16), dict(rule=2, Pr=2, pr=1, beta0=1, tpb_shift=1)):
        assert gemm_plan(hk, **ok) == _lib.GOGP_OK, ok


def syrk(hk, bs=256, ld=32, K=32, l_off=0, row_stride=None, nblocks=1, l_len=None, d_len=None):
    row_stride = bs * ld if row_stride is None else row_stride
    l_len = l_len or l_off + (nblocks - 1) * row_stride + (bs - 1) * ld + K
    d_len = d_len or nblocks * bs * bs
    L, D = np.zeros(l_len, np.float32), np.zeros(d_len)
    return hk.gogp_test_diag_syrk(-1, bs, L.ctypes.data, l_len, l_off, ld, K, row_stride,
                                  D.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), d_len, nblocks)


@pytest.mark.parametrize("bad", [dict(K=8), dict(K=0), dict(K=24, ld=32), dict(bs=128), dict(ld=30),
                                 dict(l_off=2), dict(nblocks=0), dict(row_stride=255 * 32),
                                 dict(bs=512, row_stride=6), dict(l_len=100), dict(d_len=256 * 256 - 1),
                                 dict(bs=512, nblocks=2, row_stride=600 * 32, l_len=600 * 32 + 511 * 32)],
                         ids=str)
def test_diag_syrk_hook_refuses(hk, bad):
    assert syrk(hk, **bad) == _lib.GOGP_EARG


def test_diag_syrk_hook_accepts_k16(hk):
    assert syrk(hk, K=16, ld=16) in (_lib.GOGP_OK, _lib.GOGP_EHIP)


@pytest.mark.parametrize("bad", [dict(variant=4), dict(variant=-1), dict(ld=255), dict(ld=257), dict(ldl=200),
                                 dict(row0=-1), dict(nvalid=-1)], ids=str)
def test_diag256_hook_refuses(hk, bad):
    a = dict(variant=0, ld=256, ldl=256, row0=0, nvalid=256)
    a.update(bad)
    A = np.zeros((256, max(a["ld"], 256)))
    L = np.zeros((256, max(a["ldl"], 256)))
    D = np.zeros((256, 512))
    info = ctypes.c_longlong(0)
    dp = ctypes.POINTER(ctypes.c_double)
    assert hk.gogp_test_diag256_product(-1, a["variant"], A.ctypes.data_as(dp), a["ld"], L.ctypes.data_as(dp),
                                        a["ldl"], D.ctypes.data_as(dp), a["row0"], a["nvalid"],
                                        ctypes.byref(info)) == _lib.GOGP_EARG


def test_wrappers_check_coverage_before_the_hook():
    from gogp_amd import gp
    A, B, C = np.zeros((T, 32)), np.zeros((T, 32)), np.zeros((T, T))
    with pytest.raises(ValueError):
        gp.gemm_nt_check("RECT", 1, 1, 32, A, B, C, a_off=2)
    with pytest.raises(ValueError):
        gp.gemm_nt_check("RECT", 1, 1, 32, A, B, C, k=2, bstride=4096)
    with pytest.raises(ValueError):
        gp.gemm_nt_check("RECT", 1, 2, 32, A, B, C)
    with pytest.raises(TypeError):
        gp.gemm_nt_check("RECT", 1, 1, 32, A, B.astype(np.float32), C)
    with pytest.raises(TypeError):
        gp.gemm_nt_check("RECT", 1, 1, 32, A, B, C, rulez=1)
    with pytest.raises(ValueError):
        gp.diag_syrk_check(np.zeros((256, 32), np.float32), np.zeros(256 * 256), 32, 2)
    with pytest.raises(ValueError):
        gp.diag256_product(np.zeros((255, 256)))
