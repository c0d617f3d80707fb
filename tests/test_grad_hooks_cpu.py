"""CPU side of tests/test_grad_kernels.py: the hooks of the gradient reduction and of the input gradient refuse what a
launch cannot honour, or the arrays do not cover, with GOGP_EARG BEFORE touching the device (so these pass on a machine
without a GPU)."""
import numpy as np
import pytest

from gogp_amd import _lib

NACC = _lib.GOGP_TEST_NACC


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def call(gp, which="global", prec=64, ndim=3, terms=None, ard_dims=None, radial1=True, mfma_min=65, ev=False, n=100,
         npad=128, ld=None, max_blocks=0, k=1, bstride=0, x_len=None, alpha_len=None, kinv_len=None, partials_len=None,
         mrows=128, ncols=128, nb_shift=6, grid=(0, 1, 0, 1), events=(), ev_axis=0, inv_len_tail=0.0, gx_len=None):
    terms = terms or [dict(kind=0, c=1.0, inv_len=1.0)]
    kp = gp.kparams(ndim, terms, events=events, ev_axis=0)
    kp.ev_axis = ev_axis
    if inv_len_tail and ndim < 64:
        kp.inv_len[0][ndim] = inv_len_tail
    if ard_dims is None:
        ard_dims = ndim if any(t.get("ard") for t in terms) else 0
    dt = np.float64 if prec == 64 else np.float32
    rows, cols = (npad, npad) if which != "local" else (mrows, ncols)
    ld = ld if ld is not None else cols
    blocks = _lib.hooks().gogp_test_grad_blocks(npad, *((mrows, ncols) if which == "local" else (0, 0)), max(max_blocks, 0))
    blocks = max(blocks, 1)
    X = np.zeros(x_len if x_len is not None else npad * ndim + 64)
    alpha = np.zeros(alpha_len if alpha_len is not None else (k - 1) * bstride + npad)
    Kinv = np.zeros(kinv_len if kinv_len is not None else (k - 1) * bstride + max(rows - 1, 0) * max(ld, 1) + cols, dt)
    part = np.zeros(partials_len if partials_len is not None else (k - 1) * bstride + blocks * NACC)
    out = np.zeros(k * NACC)
    H, dp = _lib.hooks(), gp._dp
    kps = (_lib.CKParams * k)(*([kp] * k))
    if which == "global":
        return H.gogp_test_grad_reduce(-1, prec, kps, ard_dims, int(radial1), mfma_min, int(ev), dp(X), X.size, dp(alpha),
                                       alpha.size, Kinv.ctypes.data, Kinv.size, ld, n, npad, max_blocks, k, bstride, dp(part),
                                       part.size, dp(out))
    if which == "local":
        pr, Pr, pc, Pc = grid
        return H.gogp_test_grad_reduce_local(-1, prec, kps, ard_dims, int(radial1), mfma_min, int(ev), dp(X), X.size,
                                             dp(alpha), alpha.size, Kinv.ctypes.data, Kinv.size, ld, n, npad, mrows, ncols,
                                             nb_shift, pr, Pr, pc, Pc, max_blocks, k, bstride, dp(part), part.size, dp(out))
    gx = np.zeros(gx_len if gx_len is not None else npad * ndim)
    return H.gogp_test_xgrad(-1, kps, int(ev), dp(X), X.size, dp(alpha), alpha.size, dp(Kinv), Kinv.size, ld, n, npad,
                             dp(gx), gx.size)


ARD = [dict(kind=0, ard=True, inv_len=[1.0, 2.0, 3.0])]
BIG = 128 * 128
REFUSED = [
    dict(prec=16),
    dict(x_len=128 * 3 + 63),                     # the zeroed slack behind X is part of the contract
    dict(alpha_len=127),
    dict(kinv_len=127 * 128 + 127),
    dict(partials_len=3 * NACC - 1),              # npad 128: 3 lower tiles
    dict(ld=127),                                 # ld < npad
    dict(n=129),                                  # n > npad
    dict(n=0),
    dict(npad=96, n=90),                          # npad not a multiple of 64
    dict(npad=0),
    dict(ard_dims=2),                             # ard_dims is 0 or ndim
    dict(terms=ARD, ard_dims=0),                  # ... and ndim exactly when a term is ARD
    dict(ard_dims=3),
    dict(terms=ARD, ev=True, events=[(0.1, 0.2, 0.5)]),   # no instance has events and ARD
    dict(terms=[dict(kind=0), dict(kind=1)], radial1=True),
    dict(terms=[dict(kind=4, w=1.0)], radial1=True),      # a periodic term is not radial
    dict(terms=[dict(kind=5)], radial1=False),
    dict(terms=[dict(kind=0, ard=True), dict(kind=1, ard=True)], radial1=False),   # one ARD term at most
    dict(inv_len_tail=1.0),                       # inv_len beyond ndim must be 0: the ARD pass multiplies by it
    dict(ev_axis=3),
    dict(mfma_min=0),
    dict(max_blocks=-1),
    dict(k=0),
    dict(k=17, bstride=BIG),
    dict(k=2, bstride=BIG, prec=32),              # candidates are the fp64 path's
    dict(k=2, bstride=BIG - 64),                  # the slots would overlap
    dict(k=2, bstride=0),
    dict(which="local", k=2, bstride=BIG),        # the local launcher has no candidate batch
    dict(which="local", mrows=96),
    dict(which="local", ncols=0),
    dict(which="local", ld=64),                   # ld < ncols
    dict(which="local", grid=(2, 2, 0, 1)),       # pr outside the grid
    dict(which="local", grid=(0, 1, 0, 0)),
    dict(which="local", nb_shift=5),              # a 64-tile would straddle distribution blocks
    dict(which="local", grid=(1, 2, 0, 1), npad=128),   # the rank's last row lies beyond npad
    dict(which="local", kinv_len=127 * 128),
    dict(which="local", partials_len=4 * NACC - 1),
    dict(which="local", max_blocks=-2),
    dict(which="local", n=200),
    dict(which="xgrad", gx_len=128 * 3 - 1),
    dict(which="xgrad", x_len=128 * 3 - 1),
    dict(which="xgrad", ld=100),
    dict(which="xgrad", npad=100),
    dict(which="xgrad", n=0),
    dict(which="xgrad", alpha_len=64),
    dict(which="xgrad", kinv_len=128 * 128 - 1),
]


@pytest.mark.parametrize("bad", REFUSED, ids=[",".join("%s=%s" % (k, v if k != "terms" else len(v)) for k, v in d.items())
                                              for d in REFUSED])
def test_grad_hooks_refuse(gpm, bad):
    assert call(gpm, **bad) == _lib.GOGP_EARG


def test_grad_hooks_accept_the_valid_neighbours(gpm):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for ok in (dict(), dict(prec=32), dict(terms=ARD), dict(terms=ARD, mfma_min=1), dict(ld=130), dict(n=128),
               dict(ev=True, events=[(0.1, 0.2, 0.5)], ev_axis=2), dict(max_blocks=2), dict(k=2, bstride=BIG),
               dict(which="local"), dict(which="local", grid=(1, 2, 0, 1), npad=256, n=200), dict(which="xgrad"),
               dict(which="xgrad", terms=ARD, ev=True)):
        assert call(gpm, **ok) in (_lib.GOGP_OK, _lib.GOGP_EHIP), ok


def test_grad_blocks(gpm):
    assert gpm.grad_blocks(256) == 10 and gpm.grad_blocks(256, 3) == 3 and gpm.grad_blocks(256, 99) == 10
    assert gpm.grad_blocks(8192) == 2048                       # GR_BLOCKS_MAX
    assert gpm.grad_blocks(512, 0, 512, 1024) == 128 and gpm.grad_blocks(512, 1, 512, 1024) == 1
    for bad in ((100, 0, 0, 0), (256, -1, 0, 0), (256, 0, 100, 128), (256, 0, 0, 128)):
        npad, mb, mr, nc = bad
        with pytest.raises(gpm.GogpError):
            gpm.grad_blocks(npad, mb, mr, nc)


def test_wrappers_check_types_before_the_hook(gpm):
    kp = gpm.kparams(1, [dict(kind=0)])
    z = np.zeros
    with pytest.raises(TypeError):
        gpm.grad_reduce_check(kp, z(128 + 64, np.float32), z(64), z(64 * 64), 64, 64, 64, z(NACC), z(NACC))
    with pytest.raises(ValueError):
        gpm.grad_reduce_check(kp, z(128 + 64), z(64), z(64 * 64), 64, 64, 64, z(NACC), z(NACC + 1))
    with pytest.raises(ValueError):
        gpm.kparams(65, [dict(kind=0)])
    with pytest.raises(gpm.GogpError):
        gpm.grad_reduce_check(kp, z(10), z(64), z(64 * 64), 64, 64, 64, z(NACC), z(NACC))
