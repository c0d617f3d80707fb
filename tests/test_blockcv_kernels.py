"""The two kernels of leave-block-out cross-validation (blockcv.hip) in isolation, through their product launchers via
gogp_test_blockcv_groups and gogp_test_blockcv_apply (include/gogp_testhooks.h); run with -m gpu.

The group kernel (one in-LDS factorisation per group of blocks of K^-1's diagonal) against numpy per block
(blockcv_ref.block_terms / sqrt_factor).  Its input is a random symmetric matrix Q = I + G G^T / (4 n) with G standard
normal: eigenvalues in [1, ~2.5], so cond(Q) < 3 and so is every diagonal block's; a Cholesky factor, its inverse and the
dot products behind w, v and the column norms of at most 128 terms then carry a few hundred roundings of 1.1e-16 each.
Bound: every quantity within 1e-11 of the largest absolute value of its reference (two orders above that estimate, nine
below a wrong element).  Q sits in the lower triangle with NaN above the diagonal and in the padding of its rows: only
j <= i < n may be read.  S_g must be exactly zero off its blocks.

The block multiply against the product in long double, per element within gamma_k (|A| |S|), k = 128 + 2,
gamma_k = k u / (1 - k u), u = 2^-53: the bound of a 128-term fp64 dot product however it is ordered or fused.  Groups
start at odd columns (no 16-byte alignment of a slice's rows), the matrix itself starts at an odd element of its
buffer; guard rows before and behind it, the padding of its rows and the columns >= n keep their bits."""
import ctypes

import numpy as np
import pytest

import blockcv_ref as BR
from gogp_amd import _lib

pytestmark = pytest.mark.gpu
I64P = ctypes.POINTER(ctypes.c_int64)
DP = ctypes.POINTER(ctypes.c_double)
U = 2.0 ** -53


def _dp(a):
    return a.ctypes.data_as(DP)


def _ip(a):
    return a.ctypes.data_as(I64P)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _sent(k):
    """NaNs with a payload: what a launch must not write (and, read, would poison a result)"""
    return (np.uint64(0x7FF8_0000_0000_0000) + np.arange(1, k + 1, dtype=np.uint64)).view(np.float64).copy()


def _problem(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    Q = np.eye(n) + G @ G.T / (4.0 * n)
    return Q, rng.standard_normal(n), rng.standard_normal(n)


def _run_groups(Q, alpha, y, start, tail=5):
    n, F = len(y), len(start) - 1
    ld = n + 3
    Kin = _sent(n * ld).reshape(n, ld)
    il = np.tril_indices(n)
    Kin[il] = Q[il]
    first = BR.groups(start)
    ng = len(first) - 1
    out = []
    for _ in range(2):
        mu, sigma, v, ones = (_sent(n + tail) for _ in range(4))
        logp, Sg = _sent(F + tail), _sent(ng * 128 * 128 + tail)
        info = np.full(ng + tail, -5, dtype=np.int64)
        st = np.asarray(start, dtype=np.int64)
        rc = _lib.hooks().gogp_test_blockcv_groups(0, _dp(Kin), Kin.size, ld, _dp(alpha), n, _dp(y), n, n, _ip(st), F,
                                                   _dp(mu), mu.size, _dp(sigma), sigma.size, _dp(v), v.size, _dp(ones),
                                                   ones.size, _dp(logp), logp.size, _dp(Sg), Sg.size, _ip(info), info.size)
        assert rc == _lib.GOGP_OK
        out.append((mu, sigma, v, ones, logp, Sg, info))
    for a, b in zip(*out):  # two identical launches: the same bits
        np.testing.assert_array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
    mu, sigma, v, ones, logp, Sg, info = out[0]
    for a, k in ((mu, n), (sigma, n), (v, n), (ones, n), (logp, F), (Sg, ng * 128 * 128)):
        np.testing.assert_array_equal(_bits(a[k:]), _bits(_sent(len(a))[k:]))  # nothing behind the arrays is written
    assert (info[ng:] == -5).all()
    return mu[:n], sigma[:n], v[:n], ones[:n], logp[:F], Sg[:ng * 128 * 128].reshape(ng, 128, 128), info[:ng], first


GROUP_CASES = {
    "n1": (1,),
    "n20": (7, 13),
    "n128_one": (128,),
    "n128_ones": (1,) * 128,
    "n200": (63, 2, 64, 71),
}


@pytest.mark.parametrize("name", sorted(GROUP_CASES))
def test_group_kernel(name):
    lengths = GROUP_CASES[name]
    start = BR.starts(lengths)
    n = int(start[-1])
    Q, alpha, y = _problem(n, 7 + n)
    mu, sigma, v, ones, logp, Sg, info, first = _run_groups(Q, alpha, y, start)
    assert not info.any()
    np.testing.assert_array_equal(ones, np.ones(n))
    want_mu, want_sigma, want_v, want_logp = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(len(lengths))
    want_S = np.zeros_like(Sg)
    inblock = np.zeros(Sg.shape, dtype=bool)
    for g in range(len(first) - 1):
        c0 = int(start[first[g]])
        for f in range(first[g], first[g + 1]):
            a, b = int(start[f]), int(start[f + 1])
            C, X, w, vb = BR.block_terms(Q, alpha, a, b)
            want_mu[a:b] = y[a:b] - vb
            want_sigma[a:b] = np.sqrt(np.diag(X.T @ X))
            want_v[a:b] = vb
            want_logp[f] = -0.5 * w @ w + np.log(np.diag(C)).sum() - 0.5 * (b - a) * BR.LOG_2PI
            want_S[g, a - c0:b - c0, a - c0:b - c0] = BR.sqrt_factor(X, w, vb)
            inblock[g, a - c0:b - c0, a - c0:b - c0] = True
    for what, got, want in (("mu", mu, want_mu), ("sigma", sigma, want_sigma), ("v", v, want_v), ("logp", logp, want_logp),
                            ("S_g", Sg, want_S)):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print("%s %s: max |err| = %.3e of %.3e (%.2e relative; bound 1e-11)" % (name, what, err, scale, err / scale))
        assert np.isfinite(got).all() and err <= 1e-11 * scale, (name, what)
    assert (_bits(Sg[~inblock]) == 0).all(), "S_g is not exact +0.0 off its blocks"


def test_group_kernel_reports_the_first_failing_pivot():
    start = BR.starts((7, 13))
    Q, alpha, y = _problem(20, 3)
    Q[9, 9] = -1.0  # row 9: the third row of the second block; rows 7 and 8 factor
    *_, info, _ = _run_groups(Q, alpha, y, start)
    assert list(info) == [10]


def _gamma(k):
    return k * U / (1.0 - k * U)


#: npad (= the rows handed over) -> (n, block lengths): the groups start at the odd columns 65, 129 and 127, 255
APPLY_CASES = {256: (200, (63, 2, 64, 71)), 384: (333, (127, 3, 125, 77, 1))}


@pytest.mark.parametrize("npad", sorted(APPLY_CASES))
def test_block_multiply(npad):
    n, lengths = APPLY_CASES[npad]
    start = BR.starts(lengths)
    assert start[-1] == n and -(-n // 64) * 64 == npad
    first = BR.groups(start)
    ng = len(first) - 1
    assert ng == 3 and all(int(start[first[g]]) % 2 == 1 for g in (1, 2))
    rng = np.random.default_rng(npad)
    Sg = np.zeros((ng, 128, 128))
    for g in range(ng):
        c0 = int(start[first[g]])
        for f in range(first[g], first[g + 1]):
            a, b = int(start[f]) - c0, int(start[f + 1]) - c0
            Sg[g, a:b, a:b] = rng.standard_normal((b - a, b - a))
    ld, guard = npad + 9, 3
    q_off = guard * ld + 1
    A = np.zeros((npad, npad))
    A[:, :n] = rng.standard_normal((npad, n))
    A[n:, :] = 0.0  # as launch_loo_scale_symv leaves K^-1: exact zeros from row / column n on
    buf0 = _sent(q_off + npad * ld + guard * ld)
    view0 = buf0[q_off:q_off + npad * ld].reshape(npad, ld)
    view0[:, :npad] = A
    st = np.asarray(start, dtype=np.int64)
    outs = []
    for _ in range(2):
        buf = buf0.copy()
        rc = _lib.hooks().gogp_test_blockcv_apply(0, _dp(buf), buf.size, q_off, ld, npad, n, _ip(st), len(lengths),
                                                  _dp(Sg), Sg.size)
        assert rc == _lib.GOGP_OK
        outs.append(buf)
    np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]))  # two runs: the same bits
    got = outs[0][q_off:q_off + npad * ld].reshape(npad, ld)
    # guard rows, the odd element in front, the padding of the rows: bit for bit as they were
    keep = np.ones(buf0.size, dtype=bool)
    keep[q_off:q_off + npad * ld].reshape(npad, ld)[:, :npad] = False
    np.testing.assert_array_equal(_bits(outs[0])[keep], _bits(buf0)[keep])
    assert (_bits(got[:, n:npad]) == 0).all(), "columns >= n are not exact zeros any more"
    worst = 0.0
    for g in range(ng):
        c0, c1 = int(start[first[g]]), int(start[first[g + 1]])
        m = c1 - c0
        want = A[:, c0:c1].astype(np.longdouble) @ Sg[g, :m, :m].astype(np.longdouble)
        bound = _gamma(130) * (np.abs(A[:, c0:c1]) @ np.abs(Sg[g, :m, :m]))
        err = np.abs(got[:, c0:c1].astype(np.longdouble) - want).astype(np.float64)
        live = bound > 0
        ratio = (err[live] / bound[live]).max()
        worst = max(worst, ratio)
        print("npad %d group %d (columns %d .. %d): max |err| / (gamma_130 |A| |S|) = %.4f" % (npad, g, c0, c1 - 1, ratio))
        assert np.isfinite(got[:, c0:c1]).all() and (err <= bound).all()
        assert (_bits(got[n:, c0:c1]) == 0).all()  # the rows >= n: zeros times S_g
    print("RATIO blockcv_apply npad%d %.4f" % (npad, worst))


def test_hooks_refuse_what_the_launch_cannot_honour():
    Q, alpha, y = _problem(20, 3)
    st = np.array([0, 7, 19], dtype=np.int64)  # start[F] != n
    z = np.zeros(2 * 128 * 128)
    v = np.zeros(20)
    info = np.zeros(2, dtype=np.int64)
    H = _lib.hooks()
    assert H.gogp_test_blockcv_groups(0, _dp(Q), Q.size, 20, _dp(alpha), 20, _dp(y), 20, 20, _ip(st), 2, _dp(v), 20, _dp(v),
                                      20, _dp(v), 20, _dp(v), 20, _dp(v), 20, _dp(z), z.size, _ip(info), 2) == _lib.GOGP_EARG
    st = np.array([0, 7, 20], dtype=np.int64)
    buf = np.zeros(64 * 24)
    assert H.gogp_test_blockcv_apply(0, _dp(buf), buf.size, 0, 24, 64, 20, _ip(st), 2, _dp(z), 100) == _lib.GOGP_EARG  # Sg short
    assert H.gogp_test_blockcv_apply(0, _dp(buf), buf.size, 0, 24, 60, 20, _ip(st), 2, _dp(z), z.size) == _lib.GOGP_EARG
    assert H.gogp_test_blockcv_apply(0, _dp(buf), buf.size, 24, 24, 64, 20, _ip(st), 2, _dp(z), z.size) == _lib.GOGP_EARG
