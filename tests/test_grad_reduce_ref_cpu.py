"""tests/grad_reduce_ref.py against independent evidence, without a GPU: the oracle's gradient (its own pair loops and
LAPACK), a Python-int evaluation of exact mode, the events case study's discount walk, and the error bound against a
plain float64 run of the same formulas."""
import numpy as np
import pytest

import events_ref
import grad_reduce_ref as R
from cases import CASES
from gogp_amd import kernel
from gogp_amd.kernel import build_desc
from oracle import oracle

N = 50
_ARD3 = ("ard_matern32", 3, kernel.Scaled(kernel.ARD(kernel.Matern32, 3)), kernel.UniformNoise, [1.3, 0.7, 1.1, 0.9], [0.2])
ORACLE_CASES = [c for c in CASES if c[0] in ("normal1d", "scaled_rbf", "ard_rbf", "matern32", "matern52_ref",
                                             "matern52_textbook", "periodic", "hyperpriors")] + [_ARD3]


def _problem(ndim, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, ndim))
    y = np.sin(2 * np.pi * X).sum(1) + 0.1 * rng.normal(size=N)
    return X, y


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_slots_assemble_to_the_oracle_gradient(case):
    """grad[p] = 0.5 * slot(p) for every similarity parameter and 0.5 * trace * dnoise for the noise one
    (dnoise = d noise_var / d log std = 2 noise_var), as assemble_gradient maps them; alpha and K^-1 from numpy."""
    name, ndim, simil, noise, ts, tn = case
    X, y = _problem(ndim, 5)
    desc = build_desc(ndim, simil, noise)
    o = oracle.FastOracle(ndim, simil, noise, use_c=False)
    o.Absorb(X, y, ts, tn)
    want = o.Gradient()
    kp = R.kp_from_desc(desc, ts, tn)
    K = oracle.gram_np(desc, np.asarray(ts, float), X, X) + kp.noise_var * np.eye(N)
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    vals, _ = R.slot_sums(kp, X, N, alpha, [Kinv])
    got = R.assemble(desc, vals[0], kp.dnoise).astype(np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (got, want)
    # the matrix-core form's model differs in the bound only
    if kp.radial1 and kp.ard_dims:
        v2, b2 = R.slot_sums(kp, X, N, alpha, [Kinv], form="mfma")
        assert np.array_equal(v2, vals) and np.all(b2 >= 0)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_float64_run_stays_inside_the_bound(case):
    name, ndim, simil, noise, ts, tn = case
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, ndim))
    alpha, Kinv = rng.normal(size=N), rng.normal(size=(N, N))
    kp = R.kp_from_desc(build_desc(ndim, simil, noise), ts, tn)
    K32 = Kinv.astype(np.float32)
    ref, bnd = R.slot_sums(kp, X, N, alpha, [Kinv, K32])
    f64, _ = R.slot_sums(kp, X, N, alpha, [Kinv, K32], mode="f64")
    assert np.all(np.abs(f64.astype(R.LD) - ref) <= bnd)
    live = bnd > 0
    assert np.all(bnd[live] <= 1e-10 * np.abs(ref).max())   # the bound cannot hide a wrong slot
    assert np.all(ref[~live] == 0)
    gref, gb = R.xgrad_sums(kp, X, N, alpha, Kinv + Kinv.T)
    g64, _ = R.xgrad_sums(kp, X, N, alpha, Kinv + Kinv.T, mode="f64")
    assert np.all(np.abs(g64.astype(R.LD) - gref) <= gb) and gb.max() <= 1e-10 * np.abs(gref).max()


def test_xgrad_matches_the_oracle():
    name, ndim, simil, noise, ts, tn = [c for c in CASES if c[0] == "hyperpriors"][0]
    X, y = _problem(ndim, 7)
    desc = build_desc(ndim, simil, noise)
    kp = R.kp_from_desc(desc, ts, tn)
    rng = np.random.default_rng(3)
    W = rng.normal(size=(N, N))
    W = W + W.T
    alpha = rng.normal(size=N)
    want = oracle.xgrad_np(desc, np.asarray(ts, float), X, X, W - np.diag(np.diag(W)))
    got, _ = R.xgrad_sums(kp, X, N, alpha, np.outer(alpha, alpha) - W)
    assert np.abs(got.astype(np.float64) - want.reshape(N, ndim)).max() <= 1e-9 * np.abs(want).max()


def test_exact_mode_against_python_ints():
    rng = np.random.default_rng(2)
    n = 131
    alpha = rng.integers(-4, 5, n).astype(float)
    Kinv = rng.integers(-8, 9, (n, n)).astype(float)
    kp = R.KP(2, [dict(kind=R.K_MATERN52, c=0.5), dict(kind=R.K_PERIODIC, c=4.0, w=3.0)])
    for mask in (None, R.tile_mask(n, (1, 2, 0, 2), nb=64)):
        got = R.exact_slots(kp, alpha, Kinv, n, mask)
        total, trace = 0, 0
        for i in range(n):
            for j in range(i + 1):
                if mask is None or mask[i, j]:
                    w = int(alpha[i]) * int(alpha[j]) - int(Kinv[i, j])
                    total += w * (1 if i == j else 2)
                    trace += w if i == j else 0
        assert (total, trace) == R.exact_slots(kp, alpha, Kinv, n, mask, as_object=True)
        want = np.zeros(R.NACC)
        want[0], want[3], want[R.ACC_TRACE] = 0.5 * total, 4.0 * total, trace
        assert np.array_equal(got, want)
    # ... and the long-double sums at identical inputs give the same numbers
    X = np.tile([[0.3, 0.7]], (n, 1))
    vals, bnd = R.slot_sums(kp, X, n, alpha, [Kinv])
    assert np.array_equal(vals[0].astype(np.float64), R.exact_slots(kp, alpha, Kinv, n))
    # ... and a rank's rows x cols sub-block of the pairs is its tile mask
    m = R.tile_mask(n, (1, 2, 0, 2), nb=64)
    rows, cols = np.where(m.any(1))[0], np.where(m.any(0))[0]
    sub, _ = R.slot_sums(kp, X, n, alpha, [Kinv[np.ix_(rows, cols)]], rows=rows, cols=cols)
    assert np.array_equal(sub[0].astype(np.float64), R.exact_slots(kp, alpha, Kinv, n, m))


def test_discount_rule_matches_the_events_case_study():
    rng = np.random.default_rng(4)
    events = [(1.0, 1.0, 0.5), (4.2, 6.7, 0.25), (0.5, 4.2, 0.75)]
    x = np.concatenate([rng.uniform(0, 8, 40), [1.0, 4.2, 6.7, 0.5, 1.0]])   # points on the boundaries, one twice
    got = R.discount(events, x, x)
    for i in range(len(x)):
        for j in range(len(x)):
            assert got[i, j] == events_ref.discount_pair(events, x[i], x[j])
    assert np.array_equal(got, events_ref.discount_matrix(events, x, x))
