"""The kernels of the per-observation noise variances (gogp_amd/csrc/noisevar.hip) in isolation, through their test hooks
(run with -m gpu on the MI355X box).

  * nv_diag_add_kernel: A_ii += v_i for i < n, the rows below the split on one launch and the rest on another.  One IEEE
    addition per element: held to the bit against numpy's, and every element off the diagonal and every padding row
    keeps its bits (the matrix is filled with distinct finite values, the padding diagonal included).
  * nv_gradient_kernel: dv_i = 1/2 (alpha_i^2 - Kinv_ii) on a matrix whose off-diagonal entries are NaN -- it may read the
    diagonal only -- against a long-double evaluation to 2 ulp (the kernel rounds once, by a fused multiply-add).  Rows
    that cancel to 2^-8 of alpha_i^2 are among the inputs; rows that cancel to 1e-9 of it, which the 64-bit mantissa of a
    long double no longer resolves, are held to the same 2 ulp against exact rational arithmetic.  dv behind n keeps
    its sentinels.
  * nv_append_fold_kernel, in front of append_commit_kernel as gogp_append_noisy launches them: on the exact commit
    problems of tests/update_kernels_ref.py with integer v2 added to the first part's diagonal beforehand, the fold takes
    it off again and the factor comes out bit for bit; the parts change on that diagonal only; v2 = None reproduces
    gogp_test_append_commit bit for bit.
"""
from fractions import Fraction

import numpy as np
import pytest

import update_kernels_ref as R
from cases import NAN64
from gogp_amd import gp

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 700)
AP = R.APPEND_PART
NAN_BITS = np.array([NAN64]).view(np.uint64)[0]


def npad_of(n):
    return (n + 255) // 256 * 256


def bits(a):
    return np.ascontiguousarray(a, float).reshape(-1).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("split", ["0", "512", "npad"])
@pytest.mark.parametrize("n", NS)
def test_diag_add(n, split):
    npad = npad_of(n)
    ld = npad + 8 if n == 257 else npad  # (a leading dimension beyond npad once)
    wcols = {"0": 0, "512": 512, "npad": npad}[split]
    rng = np.random.default_rng(n)
    A = rng.normal(size=(npad, ld))
    v = np.abs(rng.normal(size=n))
    v[::3] = 0.0
    got = gp.noise_variances_kernel_check("nv_diag_add", 0, A=A.reshape(-1), ld=ld, n=n, npad=npad, v=v, wcols=wcols)
    want = A.copy()
    idx = np.arange(n)
    want[idx, idx] = A[idx, idx] + v
    assert same_bits(got, want)
    # said apart: nothing off the diagonal, no padding row and none of the columns behind npad has changed
    off = np.ones((npad, ld), bool)
    off[idx, idx] = False
    assert np.array_equal(bits(got.reshape(npad, ld)[off]), bits(A[off]))


@pytest.mark.parametrize("n", NS)
def test_gradient(n):
    npad = npad_of(n)
    ld = npad
    rng = np.random.default_rng(7 * n)
    alpha = 3.0 * rng.normal(size=n)
    kd = np.abs(rng.normal(size=n)) * 10.0
    # every fourth row cancels: mildly (to 2^-8 of alpha^2, which the long double's 11 extra bits still resolve to a
    # fraction of an ulp of the result) and, every eighth, to 1e-9 of it, where only exact arithmetic is a reference
    kd[::4] = (alpha * alpha)[::4] * (1.0 + 2.0 ** -8 * rng.uniform(0.5, 1.0, size=len(kd[::4])))
    deep = np.arange(0, n, 8)
    kd[deep] = (alpha * alpha)[deep] * (1.0 + 1e-9 * rng.normal(size=len(deep)))
    Kinv = np.full((npad, ld), np.nan)
    idx = np.arange(n)
    Kinv[idx, idx] = kd
    dv = gp.noise_variances_kernel_check("nv_gradient", 0, Kinv=Kinv.reshape(-1), ld=ld, alpha=alpha, n=n, npad=npad,
                                         dv=np.full(n + 5, NAN64))
    assert np.isfinite(dv[:n]).all()
    LD = np.longdouble
    shallow = np.ones(n, bool)
    shallow[deep] = False
    want = LD(0.5) * (alpha.astype(LD) * alpha.astype(LD) - kd.astype(LD))
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    err = np.abs((dv[:n].astype(LD) - want).astype(np.float64))
    if shallow.any():
        print("nv_gradient n = %d: worst %.2f ulp against long double" % (n, (err / ulp)[shallow].max()))
    assert (err <= 2.0 * ulp)[shallow].all()
    worst = 0.0
    for i in deep:
        exact = (Fraction(float(alpha[i])) ** 2 - Fraction(float(kd[i]))) / 2
        u = Fraction(float(np.spacing(abs(float(exact)))))
        e = abs(Fraction(float(dv[i])) - exact) / u
        worst = max(worst, float(e))
        assert e <= 2, (i, float(e))
    print("nv_gradient n = %d: worst %.2f ulp against exact arithmetic on the cancelling rows" % (n, worst))
    assert (bits(dv[n:]) == NAN_BITS).all()


@pytest.mark.parametrize("ev", [False, True], ids=["plain", "ev"])
@pytest.mark.parametrize("m", [1, 63, 64])
def test_append_fold(m, ev):
    from test_update_kernels import kparams, sentinels
    nslab, n = 3, 300
    pr = R.commit_problem(m, nslab, ev, 100 * m + nslab)
    ld = n + m + 5
    X2, y2, part = pr["X2"].reshape(-1), pr["y2"], pr["part"]
    kp = kparams(gp)
    base = gp.append_commit_check(kp, X2, y2, m, n, part, nslab, sentinels((m + 1) * ld), ld, sentinels(m + 3), 0, ev)
    # v2 = None: today's launch, bit for bit, and the parts untouched
    Lnew, z2, info, pout = gp.nv_append_commit_check(kp, X2, y2, None, m, n, part, nslab, sentinels((m + 1) * ld), ld,
                                                     sentinels(m + 3), 0, ev)
    assert info == base[2] == 0 and same_bits(Lnew, base[0]) and same_bits(z2, base[1]) and same_bits(pout, part)
    # integer v2 put on the first part's diagonal beforehand: the fold takes it off again, exactly
    v2 = np.random.default_rng(m).integers(0, 9, m).astype(float)
    v2[::2] = 0.0
    shifted = part.copy()
    d = np.arange(m)
    shifted[:4096].reshape(64, 64)[d, d] += v2
    Lnew, z2, info, pout = gp.nv_append_commit_check(kp, X2, y2, v2, m, n, shifted, nslab, sentinels((m + 1) * ld), ld,
                                                     sentinels(m + 3), 0, ev)
    assert info == 0 and same_bits(Lnew, base[0]) and same_bits(z2, base[1])
    assert same_bits(pout, part)  # the diagonal is back, every other element of every part (sentinels included) kept its bits
    # ... and without the shift the variances reach S: L22 is the factor of L0 L0^T + diag(v2)
    Lnew, z2, info, _ = gp.nv_append_commit_check(kp, X2, y2, v2, m, n, part, nslab, sentinels((m + 1) * ld), ld,
                                                  sentinels(m + 3), 0, ev)
    assert info == 0
    L22 = Lnew.reshape(m + 1, ld)[:m, n:n + m]
    S = pr["L0"] @ pr["L0"].T + np.diag(v2)
    np.testing.assert_allclose(np.tril(L22) @ np.tril(L22).T, S, rtol=0, atol=64 * np.finfo(float).eps * np.abs(S).max())
