"""Batches of independent small GPs on the GPU (gogp_batch_*; diag256.hip: batch_eval_kernel, one workgroup per pair).

Every pair of a batch must give what Observe + Gradient / Produce give on a GP holding that member's data: the Gram
matrix, the factor, alpha and K^-1 are the code of the one-launch path (N <= 128), so only the order of the gradient
reduction and of the Produce sums differs.  Also: the reference's Produce known answers, event discounts, per-pair
status, bit-identity of a pair whatever else is in the batch, and the batched forecast harness (tutorial.BATCH).
"""
import io
import json
import os

import numpy as np
import pytest

import events_ref as R
from cases import ANYNOISE, CASES
from gogp_amd import _lib, kernel, priors, tutorial
from gogp_amd.gp import GP, GogpError, Model
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

NS = [0, 1, 2, 37, 127, 128]
# default_noise: ConstantNoise(1e-5) on Matern-3/2 with l = 0.3 leaves cond(K) ~ 1e11 at these sizes, and the two
# reduction orders of the gradient (and of v^T v in Produce) then differ by ~cond * eps of the largest term; the
# suite's parity tests loosen the same family for the same reason.  anynoise: a noise variance of 1e-5 on Matern-5/2
# (tutorial/anynoise) gives |alpha| ~ 1e4 at N = 128, so mu = k*^T alpha cancels to ~1e-4 of its terms: the two
# summation orders of mu differ by ~1e-11 (measured 7e-12); the gradient's sums over W = alpha alpha^T - K^-1 cancel
# the same way (measured 1.2e-11 of max|g| at N = 128); the LML stays at the base tolerance
TOL = {"default_noise": dict(lml=1e-10, grad=1e-6, prod=1e-7), "anynoise": dict(lml=1e-13, grad=1e-10, prod=1e-10)}
BASE = dict(lml=1e-13, grad=1e-11, prod=1e-12)


def _data(D, rows, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (rows, D))
    y = np.sin(1.5 * X[:, 0]) + 0.2 * X.sum(1) + 0.1 * rng.normal(size=rows)
    return X, y


def _members(rows):
    offs = [3, 0, 7, 11, rows - 128 - 1, rows - 128]
    return [(o, n) for o, n in zip(offs, NS)]


@pytest.mark.parametrize("case", CASES + [ANYNOISE], ids=lambda c: c[0])
def test_batch_matches_single_handles(case):
    name, D, simil, noise, ts, tn = case
    tol = TOL.get(name, BASE)
    rows = 140
    X, y = _data(D, rows, seed=len(name))
    mem = _members(rows)
    g = GP(D, simil, noise, device=0)
    g.set_batch(X, y, mem)
    rng = np.random.default_rng(3)
    x0 = np.log(np.array(ts + tn, dtype=float))
    xs = x0 + 0.05 * rng.normal(size=(len(mem), len(x0)))
    Zs = [rng.uniform(-2.0, 2.0, (3, D)) for _ in mem]
    lmls, grads, st = g.batch_observe_gradient(xs)
    lp, mus, sigmas, sp = g.batch_produce(xs, Zs)
    assert list(st) == [0] * len(mem) and list(sp) == [0] * len(mem)
    np.testing.assert_array_equal(lp, lmls)  # the same factorisation code in both modes
    for b, (off, n) in enumerate(mem):
        h = GP(D, simil, noise, X=X[off:off + n], Y=y[off:off + n], device=0)
        lml = h.Observe(xs[b])
        gr = h.Gradient()
        mu, sigma = h.Produce(Zs[b])
        assert abs(lmls[b] - lml) <= tol["lml"] * max(abs(lml), 1e-300), (name, n, lmls[b], lml)
        if n == 0:
            assert lmls[b] == 0.0 and not grads[b].any() and not mus[b].any()
        scale = max(np.abs(gr).max(), 1e-300)
        assert np.abs(grads[b] - gr).max() <= tol["grad"] * scale, (name, n, grads[b], gr)
        np.testing.assert_allclose(mus[b], mu, rtol=0, atol=tol["prod"] * max(1.0, np.abs(mu).max()), err_msg=name)
        np.testing.assert_allclose(sigmas[b], sigma, rtol=0, atol=tol["prod"] * max(1.0, np.abs(sigma).max()),
                                   err_msg=name)
        # ... and within the suite's oracle tolerances
        if n > 0:
            o = Oracle(D, simil, noise)
            o.set_data(X[off:off + n], y[off:off + n])
            lo = o.Observe(xs[b])
            assert abs(lmls[b] - lo) <= 1e-8 * max(1.0, abs(lo)), (name, n)
            go = o.Gradient()
            assert np.abs(grads[b] - go).max() <= 1e-6 * max(1.0, np.abs(go).max()), (name, n)
            mo, so = o.Produce(Zs[b])
            np.testing.assert_allclose(mus[b], mo, rtol=1e-6, atol=1e-8, err_msg=name)
            np.testing.assert_allclose(sigmas[b], so, rtol=1e-6, atol=1e-8, err_msg=name)
        h.close()
    g.close()


def test_produce_known_answers_through_the_batch(golden_dir):
    """gp/gp_test.go:23-120 (tests/golden/gp_test_known_answers.json), every case a member of one batch; sigma is not
    clamped: the zero-noise 'self' cases come out as they do through GP.Produce."""
    with open(os.path.join(golden_dir, "gp_test_known_answers.json")) as f:
        cases = json.load(f)["produce"]
    for c in cases:
        noise = kernel.ConstantNoise(c["noise"]["std"]) if c["noise"]["kind"] == "constant" else kernel.UniformNoise
        X = np.array(c["x"], dtype=float).reshape(-1, 1)
        y = np.array(c["y"], dtype=float)
        Z = np.array(c["z"], dtype=float).reshape(-1, 1)
        x = np.log(np.array(c["theta_simil"] + c.get("theta_noise", []), dtype=float))
        g = GP(1, kernel.Normal, noise, device=0)
        g.set_batch(X, y, [(0, len(y))])
        _, mus, sigmas, st = g.batch_produce(x[None, :], [Z])
        assert st[0] == 0, c["name"]
        h = GP(1, kernel.Normal, noise, X=X, Y=y, device=0)
        h.Observe(x)
        mu_h, sigma_h = h.Produce(Z)
        for got, want in zip(mus[0], c["mu"]):
            assert abs(got - want) <= 1e-6, (c["name"], mus[0])
        for got, want, ref in zip(sigmas[0], c["sigma"], sigma_h):
            if np.isnan(got) or np.isnan(ref):  # variance - covariance rounds around 0: the reference lets a NaN pass
                assert want == 0, c["name"]          # (gp_test.go:157), and so does the test of GP.Produce
                continue
            assert abs(got - ref) <= 1e-12, (c["name"], sigmas[0], sigma_h)
            assert abs(got - want) <= 1e-6, (c["name"], sigmas[0])
        g.close()
        h.close()


def test_events_windows_match_the_restatement(golden_dir):
    d = np.loadtxt(os.path.join(golden_dir, "events.csv"), delimiter=",")
    X, y = d[:, :1].copy(), (d[:, 1] - d[:, 1].mean()) / d[:, 1].std(ddof=1)
    simil, noise = kernel.Matern52, kernel.ScaledNoise(0.01)
    sev = kernel.Events(kernel.Scaled(simil), kernel.parse_events(R.SELFCHECK))
    g = GP(1, sev, noise, device=0)
    ends = [1, 2, 10, 25, 43]
    g.set_batch(X, y, [(0, e) for e in ends])
    rng = np.random.default_rng(2)
    xs = np.log([[1.0, 1.0, 1.0], [2.3, 0.4, 0.3], [0.6, 2.5, 1.7], [1.2, 0.8, 0.5], [2.3, 0.4, 0.3]])
    Zs = [np.array([[3.3]]), np.array([[1.0], [6.7]]), rng.uniform(0, 9, (4, 1)), np.array([[4.2]]),
          np.array([[0.9999], [6.7001]])]
    lmls, grads, st = g.batch_observe_gradient(xs)
    lp, mus, sigmas, sp = g.batch_produce(xs, Zs)
    assert not st.any() and not sp.any()
    for b, e in enumerate(ends):
        r = R.RefGP(1, kernel.parse_events(R.SELFCHECK))
        r.X, r.Y = X[:e], y[:e]
        lr = r.Observe(xs[b])
        assert abs(lmls[b] - lr) <= 1e-10 * abs(lr), (e, lmls[b], lr)
        gr = r.Gradient()
        np.testing.assert_allclose(grads[b], gr, rtol=1e-8, atol=1e-8 * np.abs(gr).max())
        mr, sr = r.Produce(Zs[b])
        np.testing.assert_allclose(mus[b], mr, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(mr).max()))
        np.testing.assert_allclose(sigmas[b], sr, rtol=1e-7, atol=1e-8)
    g.close()


def test_a_pair_does_not_depend_on_the_rest_of_the_batch():
    name, D, simil, noise, ts, tn = CASES[7]  # hyperpriors: two terms, periodic
    X, y = _data(D, 140, seed=9)
    mem = _members(140)
    g = GP(D, simil, noise, device=0)
    g.set_batch(X, y, mem)
    rng = np.random.default_rng(4)
    xs = np.log(np.array(ts + tn)) + 0.05 * rng.normal(size=(len(mem), len(ts) + len(tn)))
    Zs = [rng.uniform(-2, 2, (2, D)) for _ in mem]
    full = g.batch_observe_gradient(xs)
    fullp = g.batch_produce(xs, Zs)
    for b in range(len(mem)):
        alone = g.batch_observe_gradient(xs[b:b + 1], members=[b])
        rep = g.batch_observe_gradient(np.repeat(xs[b:b + 1], 3, axis=0), members=[b, b, b])
        sub = g.batch_observe_gradient(xs[::-1][:3], members=list(range(len(mem)))[::-1][:3])
        for got in (alone, rep):
            for r in range(len(got[0])):
                assert got[0][r].tobytes() == full[0][b].tobytes() and got[1][r].tobytes() == full[1][b].tobytes()
        if b >= len(mem) - 3:
            r = len(mem) - 1 - b
            assert sub[0][r].tobytes() == full[0][b].tobytes() and sub[1][r].tobytes() == full[1][b].tobytes()
        lp, mus, sigmas, _ = g.batch_produce(xs[b:b + 1], [Zs[b]], members=[b])
        assert lp[0].tobytes() == fullp[0][b].tobytes()
        assert mus[0].tobytes() == fullp[1][b].tobytes() and sigmas[0].tobytes() == fullp[2][b].tobytes()
    g.close()


def test_per_pair_status():
    # member 1 ends in a duplicate row of points 100 apart without noise (test_gpu_parity's construction): K holds the
    # exactly singular block [[1, 1], [1, 1]], its last pivot is exactly zero -- not positive definite
    X = 100.0 * np.arange(40, dtype=float)[:, None]
    X[-1] = X[-2]
    y = np.cos(np.arange(40.0))
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), device=0)
    mem = [(0, 20), (0, 40), (10, 20)]
    g.set_batch(X, y, mem)
    xs = np.log([[1.0], [1.0], [0.7], [np.inf]])
    lmls, grads, st = g.batch_observe_gradient(xs, members=[0, 1, 2, 2])
    assert st[1] == _lib.GOGP_ENOTPD and np.isnan(lmls[1]) and not grads[1].any()
    assert st[3] == _lib.GOGP_EARG and np.isnan(lmls[3]) and not grads[3].any()
    assert st[0] == 0 and st[2] == 0
    ok, okg, _ = g.batch_observe_gradient(xs[[0, 2]], members=[0, 2])
    assert ok.tobytes() == lmls[[0, 2]].tobytes() and okg.tobytes() == grads[[0, 2]].tobytes()
    lp, mus, sigmas, sp = g.batch_produce(xs, [X[:1]] * 4, members=[0, 1, 2, 2])
    assert list(sp) == list(st) and np.isnan(mus[1]).all() and np.isnan(sigmas[3]).all()
    with pytest.raises(GogpError):
        g.set_batch(np.zeros((129, 1)), np.zeros(129), [(0, 129)])
    with pytest.raises(GogpError):
        g.set_batch(X, y, [(30, 20)])  # past the data
    with pytest.raises(GogpError):
        g.batch_observe_gradient(xs[:1], members=[3])  # no such member
    g.close()


# ---- the batched forecast harness against the sequential one on the GPU --------------------------------------------
HYPER_SIMIL = CASES[7][2]


@pytest.fixture()
def knobs():
    names = ("OPTINP", "MINOPT", "ALG", "ITERS", "THRESHOLD", "NONORMALIZE", "OUTOFSAMPLE", "SEED", "NTASKS", "BATCH")
    saved = {k: getattr(tutorial, k) for k in names}
    yield tutorial
    for k, v in saved.items():
        setattr(tutorial, k, v)


def _run(make, golden_dir, data, ntheta, model=None, **kn):
    for k, v in dict(dict(OPTINP=False, MINOPT=0, ALG="lbfgs", ITERS=1000, THRESHOLD=1e-6, NONORMALIZE=False,
                          OUTOFSAMPLE=False, SEED=None, NTASKS=0, BATCH=False), **kn).items():
        setattr(tutorial, k, v)
    gp = make()
    out = io.StringIO()
    with open(os.path.join(golden_dir, data)) as f:
        tutorial.Evaluate(gp, model(gp) if model else gp, np.zeros(ntheta), f, out, log=io.StringIO())
    rows = [[float(v) for v in ln.split(",")] for ln in out.getvalue().strip().split("\n")]
    return rows, gp


STUDIES = [
    ("barebones.csv", lambda: GP(1, kernel.Scaled(kernel.Matern32), kernel.ScaledNoise(0.01), device=0), 3, None),
    ("hyperpriors.csv", lambda: GP(1, HYPER_SIMIL, kernel.ScaledNoise(0.01), device=0), 6,
     lambda g: Model(g, priors.HyperPriors())),
    ("events.csv", lambda: GP(1, kernel.Events(kernel.Scaled(kernel.Matern52), kernel.parse_events(R.SELFCHECK)),
                              kernel.ScaledNoise(0.01), device=0), 3, None),
]


@pytest.mark.parametrize("study", STUDIES, ids=lambda s: s[0])
def test_batched_harness_matches_the_sequential_gpu_run(knobs, golden_dir, study):
    data, make, ntheta, model = study
    want, gs = _run(make, golden_dir, data, ntheta, model, SEED=11, MINOPT=100, OUTOFSAMPLE=True)
    got, gb = _run(make, golden_dir, data, ntheta, model, SEED=11, MINOPT=100, OUTOFSAMPLE=True, BATCH=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)  # %f prints 6 decimals
    np.testing.assert_array_equal(gb.X, gs.X)
    want, _ = _run(make, golden_dir, data, ntheta, model, SEED=12, ITERS=30)
    got, _ = _run(make, golden_dir, data, ntheta, model, SEED=12, ITERS=30, BATCH=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert abs(a[5] - b[5]) <= 1e-3 * max(1.0, abs(b[5])), (data, a, b)  # final LML
        assert abs(a[2] - b[2]) <= 1e-3 * max(1.0, abs(b[2])), (data, a, b)  # forecast mean
