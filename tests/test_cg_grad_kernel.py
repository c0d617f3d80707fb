"""cg_grad_kernel (cg.hip) in isolation, through launch_cg_grad and the hook gogp_test_cg_grad (run with -m gpu on the
MI355X box): the slot sums of (scale sum_{s < S} A[s][i] B[s][j]) theta dk(x_i, x_j)/dtheta over all pairs i, j < n, the
weights formed on v_mfma_f64_16x16x4_f64.  Reference and bound: tests/cg_lml_ref.py (slot_sums_ab: long double, with
grad_reduce_ref's running-error bound and the weights' own rounding).

- n in {1, 17, 64, 65, 200} (one lane, a ragged tile, one whole tile, two tiles a side, sixteen tiles), S in {1, 3, 4, 5, 16,
  17, 64} (S not a multiple of 4: the MFMA's K padding), D in {1, 3, 8}; every family of test_cg_kernels.py's table (the
  radial kinds, periodic, the sum of four terms, the hyperpriors sum) and ARD at D = 3, 8 and 17 (one pass, one whole pass,
  three passes of 8 dimensions);
- |device - long double| <= the reference's bound, per slot; slots no parameter owns are exact zeros;
- payload NaNs in the rows of X from n on, in the columns of A and B from n on and in their rows from S on, and behind the
  NACC outputs: none reaches the result;
- `accumulate` adds to what the output holds; every launch runs twice and must return the same bits."""
import numpy as np
import pytest

import cg_lml_ref as L
import gram_ref as R
import grad_reduce_ref as G
from cases import NAN64

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
NS = [(1, 1), (17, 3), (64, 4), (65, 5), (200, 16), (65, 17), (200, 64), (17, 64), (1, 5), (64, 1)]
FAMILIES = list(R.RADIAL) + ["periodic", "max_terms", "hyperpriors"]
CASES = [(k, D) for k in FAMILIES for D in (1, 3, 8)] + [("ard", 3), ("ard", 8), ("ard", 17)]
RATIOS = {}


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def inputs(D, n, S, seed=0):
    """X with two sentinel rows, A and B as S + 1 rows of ld = n + 3: sentinels from column n on and in the last row."""
    rng = np.random.default_rng([97, D, n, S, seed])
    X = np.full((n + 2) * D, NAN64)
    X[:n * D] = rng.uniform(-1.0, 1.0, n * D)
    ld = n + 3
    A, B = np.full((S + 1, ld), NAN64), np.full((S + 1, ld), NAN64)
    A[:S, :n] = rng.standard_normal((S, n))
    B[:S, :n] = rng.standard_normal((S, n))
    return X, A, B, ld


def run(gpm, kp, X, n, A, B, ld, S, scale=1.0, out0=None, accumulate=False):
    o = np.full(G.NACC + 4, NAN64) if out0 is None else out0
    a = gpm.cg_grad_check(kp.hook(gpm), X, n, A.reshape(-1), B.reshape(-1), ld, S, o, scale=scale, accumulate=accumulate)
    b = gpm.cg_grad_check(kp.hook(gpm), X, n, A.reshape(-1), B.reshape(-1), ld, S, o, scale=scale, accumulate=accumulate)
    assert np.array_equal(bits(a), bits(b)), "two launches differ"
    assert np.array_equal(bits(a[G.NACC:]), bits(o[G.NACC:])), "behind the outputs"
    return a[:G.NACC]


def judge(kp, X, n, A, B, S, scale, got, what):
    D = kp.ndim
    want, bound = L.slot_sums_ab(kp, X[:n * D].reshape(n, D), n, A[:S], B[:S], scale)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(LD) - want).astype(F64)
    owned = bound > 0
    assert np.array_equal(got[~owned], np.zeros(int((~owned).sum()))), "%s: a slot no parameter owns is not zero" % what
    # the sums cancel (random signs), so the bound is held against the sum of the terms' magnitudes: sum |W| sum |c|
    mag = float((np.abs(scale * A[:S, :n]).T @ np.abs(B[:S, :n])).sum()) * sum(abs(T["c"]) for T in kp.terms)
    assert bound.max() <= 1e-9 * mag, "%s: the bound is too loose to judge by" % what
    ratio = float((err[owned] / bound[owned]).max()) if owned.any() else 0.0
    assert (err <= bound).all(), "%s: worst |err| / bound = %g (slot %d)" % (what, ratio, int(np.argmax(err - bound)))
    return ratio


@pytest.mark.parametrize("case", CASES, ids=["%s-D%d" % c for c in CASES])
def test_long_double(gpm, case):
    kind, D = case
    kp = R.kp_of((kind, D, 0, 0))
    worst = 0.0
    for q, (n, S) in enumerate(NS):
        X, A, B, ld = inputs(D, n, S)
        scale = (1.0, -0.25)[q % 2]
        got = run(gpm, kp, X, n, A, B, ld, S, scale)
        worst = max(worst, judge(kp, X, n, A, B, S, scale, got, "%s-D%d n %d S %d" % (kind, D, n, S)))
    RATIOS[case] = worst


def test_every_n_and_s(gpm):
    """The whole table of sizes on one family."""
    kp = R.kp_of(("matern52", 3, 0, 0))
    for n in (1, 17, 64, 65, 200):
        for S in (1, 3, 4, 5, 16, 17, 64):
            X, A, B, ld = inputs(3, n, S, seed=1)
            judge(kp, X, n, A, B, S, 1.0, run(gpm, kp, X, n, A, B, ld, S), "n %d S %d" % (n, S))


def test_more_rows_than_one_pass(gpm):
    """S = 65 and 130: the launcher's passes of 64 rows, each added behind the one before it."""
    kp = R.kp_of(("normal", 3, 0, 0))
    for S in (65, 130):
        X, A, B, ld = inputs(3, 65, S, seed=2)
        judge(kp, X, 65, A, B, S, 1.0, run(gpm, kp, X, 65, A, B, ld, S), "S %d" % S)


def test_accumulate(gpm):
    kp = R.kp_of(("max_terms", 3, 0, 0))
    n, S = 65, 5
    X, A, B, ld = inputs(3, n, S, seed=3)
    fresh = run(gpm, kp, X, n, A, B, ld, S)
    base = np.full(G.NACC + 4, NAN64)
    base[:G.NACC] = np.arange(G.NACC) - 7.0
    got = run(gpm, kp, X, n, A, B, ld, S, out0=base, accumulate=True)
    assert np.array_equal(bits(got), bits(base[:G.NACC] + fresh)), "accumulate adds the launch's sums to what was there"


def test_trace_slot_exact(gpm):
    """Integer rows: the trace slot is sum_i sum_s A[s][i] B[s][i] bit for bit, and with identical points and c a power of
    two every scale slot is c sum_ij W_ij."""
    kp = R.exact_kp("generic", 3)
    n, S = 65, 17
    rng = np.random.default_rng(5)
    X = np.tile(rng.uniform(-1, 1, 3), n)
    A, B = rng.integers(-8, 9, (S, n)).astype(F64), rng.integers(-8, 9, (S, n)).astype(F64)
    got = run(gpm, kp, X, n, A, B, n, S)
    W = A.T @ B
    assert got[G.ACC_TRACE] == np.trace(W)
    for t, T in enumerate(kp.terms):
        assert got[3 * t] == T["c"] * W.sum(), t


def test_print_the_worst_ratios():
    for c in sorted(RATIOS):
        print("cg_grad %s-D%d: worst |err| / bound = %.3g" % (c[0], c[1], RATIOS[c]))


# ---- cg_probe_kernel through launch_cg_probes ---------------------------------------------------------------------------------
PROBE_SHAPES = [(1, 0, 1), (1, 3, 4), (257, 0, 5), (256, 5, 1), (257, 17, 64), (300, 16, 3)]


@pytest.mark.parametrize("n,r,T", PROBE_SHAPES, ids=["n%d-r%d-T%d" % s for s in PROBE_SHAPES])
def test_probes(gpm, n, r, T):
    """Z[t][i] = sqrt(d_i) (sum_k Ls[i][k] Xi[t][n + k] + Xi[t][i]): integers bit for bit (d a square), random inputs to
    gamma_{r+3} of the sum of the terms' magnitudes against long double; sentinels behind n in Ls, Xi and Z and in Xi's
    row T; r not a multiple of 4 and T not a multiple of the kernel's four right-hand sides per pass."""
    rng = np.random.default_rng([99, n, r, T])
    ldn, ldxi, ld = n + 2, n + r + 3, n + 5
    for integer in (True, False):
        Ls = None
        if r:
            Ls = np.full(r * ldn, NAN64).reshape(r, ldn)
            Ls[:, :n] = rng.integers(-4, 5, (r, n)) if integer else rng.standard_normal((r, n))
        d = rng.integers(1, 4, n).astype(F64) ** 2 if integer else rng.uniform(0.01, 2.0, n)
        Xi = np.full((T + 1, ldxi), NAN64)
        Xi[:T, :n + r] = rng.integers(-8, 9, (T, n + r)) if integer else rng.standard_normal((T, n + r))
        Z0 = np.full(T * ld, NAN64)
        run1 = lambda: gpm.cg_probes_check(None if Ls is None else Ls.reshape(-1), ldn, n, r, d, Xi.reshape(-1), ldxi, ld, T, Z0)  # noqa: E731
        got, again = run1(), run1()
        assert np.array_equal(bits(got), bits(again)), "two launches differ"
        Z = got.reshape(T, ld)
        assert np.array_equal(bits(Z[:, n:]), bits(np.full((T, ld - n), NAN64))), "behind n"
        L_ = np.zeros((n, 0)) if Ls is None else Ls[:, :n].T
        want = L.form_probes(L_, d, Xi[:T], LD)
        if integer:
            assert np.array_equal(Z[:, :n], want.astype(F64))
        else:
            mag = np.sqrt(d) * (np.abs(Xi[:T, n:n + r]) @ np.abs(L_).T + np.abs(Xi[:T, :n]))
            assert (np.abs(Z[:, :n].astype(LD) - want).astype(F64) <= G.gamma(r + 3) * mag * (1 + 2.0 ** -30)).all()
