"""The full Observe form of the batch on the GPU (gogp_batch_observe_full_gradient / gogp_batch_produce_full;
diag256.hip: batch_eval_kernel<.., .., true>): every pair carries its observations in its own vector,
x = [log theta | X | y], and one launch returns per pair the LML and the whole gradient -- hyperparameters, dLML/dX
(gp/gp.go:118-129) and dLML/dy = -alpha (:488-493).

Part by part, members of n in {0, 1, 2, 37, 127, 128} in one call:
  * LML and hyperparameter part: bit-equal to batch_observe_gradient on the same data (the same code on the same
    numbers);
  * output part: bit-equal to -Alpha of a single handle after Observe(full x) (both form alpha by the code of
    tiny_eval_kernel);
  * input part: against FastOracle's full form at the project's bound, 1e-7 * max(1, |part_ref|_inf)
    (tests/test_full_form_gradient.py), and against the single handle's Observe(full x) + Gradient() at the per-family
    `grad` tolerances of tests/test_batch_windows_gpu.py (the two differ in the order of the row sums only), scaled
    by the part's largest component.
The events kernel has no descriptor oracle: its reference is tests/events_ref.py with the input part written out from
its W and discount matrix.

Every family meets the bounds as they stand; no input part needed the single handle's own distance from the oracle as
its yardstick.  Measured on one MI355X, input part, worst member of each family (the test prints every member):

    family             batch - single  batch - oracle  single - oracle
                       / max |gx|      / max(1, |gx|)  / max(1, |gx|)
    normal1d            1.4e-14         1.8e-13         1.8e-13
    scaled_rbf          1.2e-14         1.5e-13         1.5e-13
    ard_rbf             1.1e-14         6.9e-14         6.9e-14
    matern32            3.3e-15         1.1e-13         1.1e-13
    matern52_ref        5.0e-15         1.1e-13         1.1e-13
    matern52_textbook   4.9e-15         1.6e-13         1.6e-13
    periodic            8.3e-14         3.9e-13         3.5e-13
    hyperpriors         5.3e-15         1.7e-13         1.7e-13
    default_noise       1.7e-14         1.5e-11         1.5e-11
    anynoise            4.7e-12         3.2e-10         3.3e-10
    ard_rbf17           4.2e-15         3.9e-14         3.9e-14
    events              2.0e-14         4.0e-13         4.0e-13
-alpha came out bit-equal to the single handle's in every member, as expected.
"""
import io
import json
import math
import os

import numpy as np
import pytest

import events_ref as R
from cases import ANYNOISE, CASES
from gogp_amd import _lib, kernel, priors, tutorial
from gogp_amd.gp import GP, Model
from oracle.oracle import FastOracle, xgrad_np

pytestmark = pytest.mark.gpu

NS = [0, 1, 2, 37, 127, 128]
# tests/test_batch_windows_gpu.py: TOL / BASE, with the reasons given there
TOL = {"default_noise": dict(lml=1e-10, grad=1e-6, prod=1e-7), "anynoise": dict(lml=1e-13, grad=1e-10, prod=1e-10)}
BASE = dict(lml=1e-13, grad=1e-11, prod=1e-12)
ORACLE_TOL = 1e-7  # tests/test_full_form_gradient.py: TOL

D17 = 17
ARD17 = ("ard_rbf17", D17, kernel.Scaled(kernel.ARD(kernel.Normal, D17)), kernel.UniformNoise,
         [1.1] + list(np.sqrt(D17 / 6.0) * (1 + np.arange(D17) / (2.0 * D17))), [0.2])
EVENTS = kernel.parse_events(R.SELFCHECK)
EV_CASE = ("events", 1, kernel.Events(kernel.Scaled(kernel.Matern52), EVENTS), kernel.ScaledNoise(0.01),
           [1.2, 0.8], [0.5])
FAMILIES = CASES + [ANYNOISE, ARD17, EV_CASE]


def _data(name, D, n, seed):
    rng = np.random.default_rng(seed)
    if name == "events":  # inputs across both events of the self-check (1.0 and 4.2 .. 6.7)
        X = np.sort(rng.uniform(0.0, 9.0, (n, 1)), axis=0)
        y = np.sin(X[:, 0]) + 0.1 * rng.normal(size=n)
        return X, y
    X = rng.uniform(0, 1, (n, D))  # tests/test_full_form_gradient.py: _data
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=n)
    return X, ((y - y.mean()) / y.std() if n > 1 else y)


def _full_x(logtheta, X, y):
    return np.concatenate([logtheta, X.reshape(-1), y])


def _pairs(case, seed=3):
    name, D, simil, noise, ts, tn = case
    rng = np.random.default_rng(seed)
    x0 = np.log(np.array(list(ts) + list(tn), dtype=float))
    data = [_data(name, D, n, 100 * len(name) + n) for n in NS]
    thetas = [x0 + 0.05 * rng.normal(size=len(x0)) for _ in NS]
    return data, thetas, [_full_x(t, X, y) for t, (X, y) in zip(thetas, data)]


def _events_reference(x, P):
    """LML and the whole full-form gradient of the events kernel from tests/events_ref.py: its W, with the pair's
    discount as a factor of W_ij in the input part (the discount is piecewise constant in x)."""
    r = R.RefGP(1, EVENTS)
    lml = r.Observe(x)
    W = np.outer(r.alpha, r.alpha) - np.linalg.inv(r.K)
    Dm = R.discount_matrix(r.events, r.X[:, 0], r.X[:, 0])
    desc = kernel.build_desc(1, kernel.Scaled(kernel.Matern52), kernel.ScaledNoise(0.01))
    gx = xgrad_np(desc, r.theta[:2], r.X, r.X, W * Dm)
    return lml, np.concatenate([r.Gradient(), gx.reshape(-1), -r.alpha])


def _reference(case, x, P):
    name, D, simil, noise, _, _ = case
    if name == "events":
        return _events_reference(x, P)
    o = FastOracle(D, simil, noise)
    return o.Observe(x), o.Gradient()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c[0])
def test_full_form_batch_part_by_part(case):
    name, D, simil, noise, ts, tn = case
    tol = TOL.get(name, BASE)
    P = len(ts) + len(tn)
    data, thetas, xs = _pairs(case)
    g = GP(D, simil, noise, device=0)
    lmls, grads, st = g.batch_observe_full_gradient(xs)
    assert list(st) == [0] * len(NS)
    # the hyperparameters-only batch on the same data: rows of one upload
    Xall = np.concatenate([X for X, _ in data], axis=0)
    yall = np.concatenate([y for _, y in data])
    offs = np.concatenate([[0], np.cumsum(NS)])[:-1]
    g.set_batch(Xall, yall, [(int(o), n) for o, n in zip(offs, NS)])
    lh, gh, sh = g.batch_observe_gradient(np.array(thetas))
    assert not sh.any()
    bad = []  # every member is measured (and printed) before the test fails
    for b, n in enumerate(NS):
        X, y = data[b]
        assert grads[b].shape == (P + n * (D + 1),)
        # LML and hyperparameter part: bit-equal
        assert lmls[b].tobytes() == lh[b].tobytes(), (name, n, lmls[b], lh[b])
        assert grads[b][:P].tobytes() == gh[b].tobytes(), (name, n, grads[b][:P], gh[b])
        if n == 0:
            assert lmls[b] == 0.0 and not grads[b].any()
            continue
        h = GP(D, simil, noise, device=0)
        lml_h = h.Observe(xs[b])
        grad_h = h.Gradient()
        alpha_h = h.Alpha
        h.close()
        gx, gx_h = grads[b][P:P + n * D], grad_h[P:P + n * D]
        lml_o, grad_o = _reference(case, xs[b], P)
        gx_o = grad_o[P:P + n * D]
        e_single = float(np.abs(gx - gx_h).max() / max(np.abs(gx_h).max(), 1e-300)) if n > 1 else 0.0
        e_oracle, e_single_oracle = _rel(gx, gx_o), _rel(gx_h, gx_o)
        e_alpha = _rel(grads[b][P + n * D:], grad_o[P + n * D:])
        print("ERR %s n=%d gx: batch-single=%.2e batch-oracle=%.2e single-oracle=%.2e |gx|=%.2e  alpha-oracle=%.2e "
              "alpha bit-equal=%s lml-single=%.2e" % (name, n, e_single, e_oracle, e_single_oracle, np.abs(gx_h).max(),
                                                      e_alpha, grads[b][P + n * D:].tobytes() == (-alpha_h).tobytes(),
                                                      abs(lmls[b] - lml_h)))
        bad += [(name, n, what) for ok, what in (
            # output part: -alpha of the single handle, bit for bit
            (grads[b][P + n * D:].tobytes() == (-alpha_h).tobytes(), "alpha differs from the single handle's"),
            (abs(lmls[b] - lml_h) <= tol["lml"] * max(abs(lml_h), 1e-300), "lml against the single handle"),
            (np.abs(grads[b][:P] - grad_h[:P]).max() <= tol["grad"] * max(np.abs(grad_h[:P]).max(), 1e-300),
             "hyperparameter part against the single handle"),
            # input part
            (bool(np.all(np.isfinite(gx))), "gx not finite"),
            (n > 1 or not gx.any(), "n = 1 has no partner: the sum over j != i is empty"),
            (np.abs(gx - gx_h).max() <= tol["grad"] * max(np.abs(gx_h).max(), 1e-300),
             "gx against the single handle: %.2e" % e_single),
            (e_oracle <= ORACLE_TOL, "gx against the oracle: %.2e (single handle: %.2e)" % (e_oracle, e_single_oracle)),
            (e_alpha <= ORACLE_TOL, "alpha against the oracle: %.2e" % e_alpha),
            (abs(lmls[b] - lml_o) <= 1e-8 * max(1.0, abs(lml_o)), "lml against the oracle"),
            (_rel(grads[b][:P], grad_o[:P]) <= ORACLE_TOL, "hyperparameter part against the oracle")) if not ok]
    g.close()
    assert not bad, bad


def test_full_form_per_pair_status_and_independence():
    name, D, simil, noise, ts, tn = CASES[7]  # hyperpriors: two terms, periodic
    P = len(ts) + len(tn)
    data, thetas, xs = _pairs(CASES[7], seed=4)
    g = GP(D, simil, noise, device=0)
    full = g.batch_observe_full_gradient(xs)
    assert not full[2].any()
    # bad pairs among the good ones: a length with a remainder, one shorter than P, n = 129, a non-finite row,
    # non-finite parameters
    X129, y129 = _data(name, D, 129, 5)
    bad_nan = xs[3].copy()
    bad_nan[P + 5] = np.nan
    bad_theta = xs[2].copy()
    bad_theta[0] = np.inf
    bad = [np.append(xs[3], 0.5), xs[1][:P - 1], _full_x(thetas[0], X129, y129), bad_nan, bad_theta]
    mixed = [bad[0], xs[0], xs[1], bad[1], xs[2], bad[2], xs[3], bad[3], xs[4], bad[4], xs[5]]
    good = [1, 2, 4, 6, 8, 10]
    lm, gr, st = g.batch_observe_full_gradient(mixed)
    for i in (0, 3, 5, 7, 9):
        assert st[i] == _lib.GOGP_EARG and np.isnan(lm[i]) and not gr[i].any() and gr[i].size == mixed[i].size
    for b, i in enumerate(good):
        assert st[i] == 0 and lm[i].tobytes() == full[0][b].tobytes() and gr[i].tobytes() == full[1][b].tobytes()
    # a pair alone, repeated, and in a permuted batch: the same bytes
    perm = [5, 2, 4, 0, 3, 1]
    pm = g.batch_observe_full_gradient([xs[b] for b in perm])
    for r, b in enumerate(perm):
        assert pm[0][r].tobytes() == full[0][b].tobytes() and pm[1][r].tobytes() == full[1][b].tobytes()
    Zs = [np.random.default_rng(6).uniform(0, 1, (2, D)) for _ in NS]
    fullp = g.batch_produce_full(xs, Zs)
    np.testing.assert_array_equal(fullp[0], full[0])  # the same factorisation code in both modes
    for b in range(len(NS)):
        alone = g.batch_observe_full_gradient([xs[b]])
        rep = g.batch_observe_full_gradient([xs[b]] * 3)
        for got in (alone, rep):
            for r in range(len(got[0])):
                assert got[0][r].tobytes() == full[0][b].tobytes() and got[1][r].tobytes() == full[1][b].tobytes()
        lp, mus, sigmas, sp = g.batch_produce_full([xs[b]], [Zs[b]])
        assert sp[0] == 0 and lp[0].tobytes() == fullp[0][b].tobytes()
        assert mus[0].tobytes() == fullp[1][b].tobytes() and sigmas[0].tobytes() == fullp[2][b].tobytes()
    lp, mus, sigmas, sp = g.batch_produce_full(mixed, [Zs[0]] * len(mixed))
    assert [int(s) for s in sp] == [int(s) for s in st]
    assert np.isnan(mus[0]).all() and np.isnan(sigmas[5]).all() and np.isnan(lp[7])
    g.close()


def test_full_form_not_positive_definite_pair():
    # tests/test_batch_windows_gpu.py::test_per_pair_status: a duplicate row of points 100 apart without noise leaves
    # the exactly singular block [[1, 1], [1, 1]] -- its last pivot is exactly zero
    X = 100.0 * np.arange(40, dtype=float)[:, None]
    X[-1] = X[-2]
    y = np.cos(np.arange(40.0))
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), device=0)
    t = np.log([1.0])
    xs = [_full_x(t, X[:20], y[:20]), _full_x(t, X, y), _full_x(np.log([0.7]), X[10:30], y[10:30])]
    lm, gr, st = g.batch_observe_full_gradient(xs)
    assert st[1] == _lib.GOGP_ENOTPD and np.isnan(lm[1]) and not gr[1].any()
    assert st[0] == 0 and st[2] == 0
    ok = g.batch_observe_full_gradient([xs[0], xs[2]])
    assert ok[0].tobytes() == lm[[0, 2]].tobytes()
    assert ok[1][0].tobytes() == gr[0].tobytes() and ok[1][1].tobytes() == gr[2].tobytes()
    lp, mus, sigmas, sp = g.batch_produce_full(xs, [X[:1]] * 3)
    assert list(sp) == list(st) and np.isnan(mus[1]).all() and np.isnan(sigmas[1]).all() and np.isnan(lp[1])
    # the handle's own state is untouched: it still holds nothing
    assert len(g.X) == 0
    g.close()


def test_full_form_refused_on_a_sharded_handle():
    import loopback
    from gogp_amd.sharded import ShardedGP
    D = 2
    simil, noise = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
    X, y = _data("m", D, 30, 1)
    x = _full_x(np.log([1.1, 0.5, 0.2]), X, y)

    def rank_fn(r, lb):
        sh = ShardedGP(D, simil, noise, device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        lml, st = np.zeros(1), np.full(1, -1, dtype=np.intc)
        grads = np.zeros(x.size)
        xoff = np.array([0, x.size], dtype=np.int64)
        import ctypes
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
        rc = _lib.lib().gogp_batch_observe_full_gradient(sh._h, 1, dp(x), xoff.ctypes.data_as(
            ctypes.POINTER(ctypes.c_int64)), dp(lml), dp(grads), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        sh.close()
        return rc, int(st[0])

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rc, st in outs:
        assert rc == _lib.GOGP_EARG and st == -1  # refused as a whole: nothing evaluated


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c[0])
def test_full_form_batch_produce_matches_single_handles(case):
    name, D, simil, noise, ts, tn = case
    tol = TOL.get(name, BASE)
    data, thetas, xs = _pairs(case, seed=8)
    rng = np.random.default_rng(9)
    Zs = [rng.uniform(0.0, 9.0 if name == "events" else 1.0, (3, D)) for _ in NS]
    g = GP(D, simil, noise, device=0)
    lmls, _, st = g.batch_observe_full_gradient(xs)
    lp, mus, sigmas, sp = g.batch_produce_full(xs, Zs)
    assert not st.any() and not sp.any()
    np.testing.assert_array_equal(lp, lmls)
    for b, n in enumerate(NS):
        h = GP(D, simil, noise, device=0)
        h.Observe(xs[b])
        mu, sigma = h.Produce(Zs[b])
        h.close()
        print("ERR produce %s n=%d mu=%.2e sigma=%.2e" % (name, n, np.abs(mus[b] - mu).max(),
                                                          np.abs(sigmas[b] - sigma).max()))
        if n == 0:
            assert not mus[b].any()
        np.testing.assert_allclose(mus[b], mu, rtol=0, atol=tol["prod"] * max(1.0, np.abs(mu).max()), err_msg=name)
        np.testing.assert_allclose(sigmas[b], sigma, rtol=0, atol=tol["prod"] * max(1.0, np.abs(sigma).max()),
                                   err_msg=name)
    g.close()


def test_full_form_produce_known_answers(golden_dir):
    """gp/gp_test.go:23-120 (tests/golden/gp_test_known_answers.json) with the observations carried in x, all cases of a
    noise level in one call; 1e-6 is the reference's bound."""
    with open(os.path.join(golden_dir, "gp_test_known_answers.json")) as f:
        cases = json.load(f)["produce"]
    assert all(c["noise"]["kind"] == "constant" for c in cases)
    for std in sorted({c["noise"]["std"] for c in cases}):
        grp = [c for c in cases if c["noise"]["std"] == std]
        noise = kernel.ConstantNoise(std)
        g = GP(1, kernel.Normal, noise, device=0)
        xs = [_full_x(np.log(np.array(c["theta_simil"] + c.get("theta_noise", []), dtype=float)),
                      np.array(c["x"], dtype=float), np.array(c["y"], dtype=float)) for c in grp]
        Zs = [np.array(c["z"], dtype=float).reshape(-1, 1) for c in grp]
        _, mus, sigmas, st = g.batch_produce_full(xs, Zs)
        for i, c in enumerate(grp):
            assert st[i] == 0, c["name"]
            for got, want in zip(mus[i], c["mu"]):
                assert abs(got - want) <= 1e-6, (c["name"], mus[i])
            for got, want in zip(sigmas[i], c["sigma"]):
                if np.isnan(got):  # variance - covariance rounds around 0: the reference lets a NaN pass
                    assert want == 0, c["name"]  # (gp_test.go:157)
                    continue
                assert abs(got - want) <= 1e-6, (c["name"], sigmas[i])
        g.close()


# ---- the batched OPTINP harness against the sequential one on the GPU ---------------------------------------------------------
@pytest.fixture()
def knobs():
    names = ("OPTINP", "MINOPT", "ALG", "ITERS", "THRESHOLD", "NONORMALIZE", "OUTOFSAMPLE", "SEED", "NTASKS", "BATCH")
    saved = {k: getattr(tutorial, k) for k in names}
    yield tutorial
    for k, v in saved.items():
        setattr(tutorial, k, v)


def _run(make, golden_dir, data, model, **kn):
    for k, v in dict(dict(OPTINP=True, MINOPT=0, ALG="lbfgs", ITERS=1000, THRESHOLD=1e-6, NONORMALIZE=False,
                          OUTOFSAMPLE=False, SEED=None, NTASKS=0, BATCH=False), **kn).items():
        setattr(tutorial, k, v)
    gp = make()
    out = io.StringIO()
    with open(os.path.join(golden_dir, data)) as f:
        tutorial.Evaluate(gp, model(gp), np.zeros(3), f, out, log=io.StringIO())
    rows = [[float(v) for v in ln.split(",")] for ln in out.getvalue().strip().split("\n")]
    return rows, gp


STUDIES = [
    ("barebones.csv", lambda: GP(1, kernel.Scaled(kernel.Matern52), kernel.ConstantNoiseParam(1e-5 ** 0.5), device=0),
     lambda g: priors.AnyNoiseModel(Model(g, priors.AnyNoisePriors()))),
    ("events.csv", lambda: GP(1, kernel.Scaled(kernel.Matern52), kernel.ScaledNoise(0.01), device=0),
     lambda g: priors.WarpedTimeModel(Model(g, priors.WarpedTimePriors(math.log(0.5))))),
]


@pytest.mark.parametrize("study", STUDIES, ids=["anynoise", "warpedtime"])
def test_batched_optinp_harness_matches_the_sequential_gpu_run(knobs, golden_dir, study):
    """The bounds of test_batch_windows_gpu.py::test_batched_harness_matches_the_sequential_gpu_run."""
    data, make, model = study
    want, gs = _run(make, golden_dir, data, model, SEED=11, MINOPT=100, OUTOFSAMPLE=True)
    got, gb = _run(make, golden_dir, data, model, SEED=11, MINOPT=100, OUTOFSAMPLE=True, BATCH=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)  # %f prints 6 decimals
    np.testing.assert_array_equal(gb.X, gs.X)
    want, _ = _run(make, golden_dir, data, model, SEED=12, ITERS=30)
    got, _ = _run(make, golden_dir, data, model, SEED=12, ITERS=30, BATCH=True)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        print("ROW lml %.6f %.6f mu %.6f %.6f" % (a[5], b[5], a[2], b[2]))
    for a, b in zip(got, want):
        assert abs(a[5] - b[5]) <= 1e-3 * max(1.0, abs(b[5])), (data, a, b)  # final LML
        assert abs(a[2] - b[2]) <= 1e-3 * max(1.0, abs(b[2])), (data, a, b)  # forecast mean
