"""hess_kmm_kernel alone, through the hook gogp_test_hess_kmm (run with -m gpu): M_q = K^-1 K_q for the value and the length
slot of Scaled(Matern32) in two dimensions at N = 129 (npad = 192: a ragged k-step, tiles on, left and right of the
diagonal) against the long-double product.  K_q is written out here from the closed forms c (1 + a r) e^(-a r) and
3 c r^2 e^(-a r), a = sqrt(3); the bound is N eps |K^-1|_F |K_q|_F on the Frobenius norm of the error.  The upper triangle
of the K^-1 handed in is NaN: only the stored half may be read."""
import numpy as np
import pytest

import grad_reduce_ref as G
import hessian_ref as R
from gogp_amd import gp as gpm
from gogp_amd import hessian, kernel

pytestmark = pytest.mark.gpu
LD = np.longdouble


def test_kmm_against_long_double():
    n, npad = 129, 192
    D, simil, noise, X, _, x = R.data("matern32", n)
    c, ell, sd = np.exp(x)
    desc = kernel.build_desc(D, simil, noise)
    kp = G.kp_from_desc(desc, [c, ell], [sd])
    Xl = X.astype(LD)
    r2 = (((Xl[:, None, :] - Xl[None, :, :]) / LD(ell)) ** 2).sum(-1)
    a = LD(G.SQRT3)
    e = np.exp(-a * np.sqrt(r2))
    Kq = [LD(c) * (1 + a * np.sqrt(r2)) * e, 3 * LD(c) * r2 * e]
    K = (Kq[0] + LD(sd) ** 2 * np.eye(n)).astype(np.float64)
    Kinv = np.linalg.inv(K)
    Kinv = (Kinv + Kinv.T) / 2
    stored = np.where(np.tril(np.ones((n, n), bool)), Kinv, np.nan)
    M = hessian.kmm_check(kp.hook(gpm), 0, [hessian.VALUE, hessian.LEN], [0, 0], X, n, npad, stored, n,
                          np.full((2, npad, npad), np.nan))
    for q in range(2):
        ref = Kinv.astype(LD) @ Kq[q]
        err = float(np.linalg.norm((M[q, :n, :n] - ref).astype(np.float64)))
        bound = n * 2.0 ** -52 * np.linalg.norm(Kinv) * float(np.linalg.norm(Kq[q].astype(np.float64)))
        print("slot %d: |M - ref|_F = %.3e, bound %.3e" % (q, err, bound))
        assert err <= bound
        pad = M[q].copy()
        pad[:n, :n] = 0.0
        assert not pad.any()  # whole tiles written, exact zeros from row / column n on
