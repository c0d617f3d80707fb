"""The batched forecast harness (tutorial.BATCH) and optimize.lbfgs_lockstep, on the CPU.

tutorial.BATCH evaluates the windows of the forecast harness (tutorial/tutorial.go:88-197) as batches of small GPs:
GP.set_batch / batch_observe_gradient / batch_produce, with the windows' L-BFGS runs in lock-step.  Behind an
oracle-backed adapter (one CPU oracle per member, so every value is the one the sequential harness computes) it must
write the SAME TEXT as the sequential harness, byte for byte, for the same SEED.
"""
import io
import os

import numpy as np
import pytest

from gogp_amd import kernel, optimize, priors, tutorial
from gogp_amd.gp import Model
from oracle.oracle import NotPositiveDefinite, Oracle

SIMIL = kernel.Scaled(kernel.Matern32)
NOISE = kernel.ScaledNoise(0.01)
HYPER_SIMIL = kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))],
                         order=[0, 2, 1, 3, 4])


class BatchOracleGP:
    """The CPU oracle with gp.GP's field / method shape (as tests/test_tutorial.py::OracleGP) plus the three batch
    methods, each member backed by an oracle of its own.  Counts what the harness calls."""

    def __init__(self, ndim, simil, noise):
        self.args = (ndim, simil, noise)
        self.o = Oracle(ndim, simil, noise)
        self.NDim = ndim
        self.X = np.zeros((0, ndim))
        self.Y = np.zeros(0)
        self.Parallel = False
        self._P = self.o.ns + self.o.nn
        self.calls = {"Observe": 0, "set_batch": 0, "batch_observe_gradient": 0, "batch_produce": 0}
        self.members = []

    def Observe(self, x):
        self.calls["Observe"] += 1
        x = np.asarray(x, dtype=float)
        if x.size == self._P:
            self.o.set_data(self.X, self.Y)
        else:  # gp/gp.go:391-396: X, Y are re-sliced out of x
            n = (x.size - self._P) // (self.NDim + 1)
            self.X = x[self._P:self._P + n * self.NDim].reshape(n, self.NDim).copy()
            self.Y = x[self._P + n * self.NDim:].copy()
            self.o.set_data(np.zeros((0, self.NDim)), np.zeros(0))
        return self.o.Observe(x)

    def Gradient(self):
        return self.o.Gradient()

    def Produce(self, Z):
        return self.o.Produce(Z)

    # ---- the batch methods of gp.GP ------------------------------------------------------------------
    def set_batch(self, X, Y, members):
        self.calls["set_batch"] += 1
        self.members = []
        for off, n in members:
            assert 0 <= n <= 128
            o = Oracle(*self.args)
            o.set_data(np.asarray(X)[off:off + n], np.asarray(Y)[off:off + n])
            self.members.append((off, n, o))

    def _members(self, k, members):
        return list(range(k)) if members is None else list(members)

    def batch_observe_gradient(self, xs, members=None):
        self.calls["batch_observe_gradient"] += 1
        xs = np.atleast_2d(xs)
        mem = self._members(len(xs), members)
        lmls, grads, st = np.zeros(len(xs)), np.zeros((len(xs), self._P)), np.zeros(len(xs), dtype=int)
        for i, (x, b) in enumerate(zip(xs, mem)):
            o = self.members[b][2]
            try:
                lmls[i] = o.Observe(x)
                grads[i] = o.Gradient()
            except NotPositiveDefinite:
                lmls[i], st[i] = np.nan, 2
        return lmls, grads, st

    def batch_produce(self, xs, Zs, members=None):
        self.calls["batch_produce"] += 1
        xs = np.atleast_2d(xs)
        mem = self._members(len(xs), members)
        lmls, mus, sigmas, st = np.zeros(len(xs)), [], [], np.zeros(len(xs), dtype=int)
        for i, (x, b) in enumerate(zip(xs, mem)):
            o = self.members[b][2]
            try:
                lmls[i] = o.Observe(x)
                mu, sigma = o.Produce(Zs[i])
            except NotPositiveDefinite:
                lmls[i], st[i] = np.nan, 2
                mu = sigma = np.full(len(Zs[i]), np.nan)
            mus.append(mu)
            sigmas.append(sigma)
        return lmls, mus, sigmas, st


@pytest.fixture()
def knobs():
    names = ("OPTINP", "MINOPT", "ALG", "ITERS", "THRESHOLD", "RATE", "NONORMALIZE", "OUTOFSAMPLE", "SEED", "NTASKS",
             "BATCH")
    saved = {k: getattr(tutorial, k, None) for k in names}
    yield tutorial
    for k, v in saved.items():
        setattr(tutorial, k, v)


DEFAULTS = dict(OPTINP=False, MINOPT=0, ALG="lbfgs", ITERS=1000, THRESHOLD=1e-6, RATE=0.01, NONORMALIZE=False,
                OUTOFSAMPLE=False, SEED=None, NTASKS=0, BATCH=False)


def _run(make, rdr_text, ntheta, model=None, **kn):
    """(output text, the GP after the run, log text)"""
    for k, v in dict(DEFAULTS, **kn).items():
        setattr(tutorial, k, v)
    gp = make()
    m = model(gp) if model else gp
    out, log = io.StringIO(), io.StringIO()
    tutorial.Evaluate(gp, m, np.zeros(ntheta), io.StringIO(rdr_text), out, log=log)
    return out.getvalue(), gp, log.getvalue()


def _same_text(make, text, ntheta, model=None, **kn):
    seq, gs, log_s = _run(make, text, ntheta, model, BATCH=False, **kn)
    bat, gb, log_b = _run(make, text, ntheta, model, BATCH=True, **kn)
    assert gs.calls["set_batch"] == 0 and gs.calls["batch_observe_gradient"] == 0
    # the batched run went through the batch methods: one set_batch, one call for the initial LMLs and one per
    # lock-step round, one forecast call
    assert gb.calls["set_batch"] == 1 and gb.calls["batch_produce"] == 1 and gb.calls["batch_observe_gradient"] >= 1
    assert bat == seq
    assert sorted(log_b.splitlines()) == sorted(log_s.splitlines())
    # the GP is left where the sequential harness leaves it
    np.testing.assert_array_equal(gb.X, gs.X)
    np.testing.assert_array_equal(gb.Y, gs.Y)
    return seq, gs, gb


def _golden(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return f.read()


def test_batched_harness_writes_the_sequential_text_barebones(knobs, golden_dir):
    text = _golden(golden_dir, "barebones.csv")
    make = lambda: BatchOracleGP(1, SIMIL, NOISE)  # noqa: E731
    seq, gs, gb = _same_text(make, text, 3, SEED=3, ITERS=30, OUTOFSAMPLE=True)
    assert len(seq.strip().split("\n")) == 20 + 19
    # every window went through the batch (the sequential code observes the GP once, to leave it at the last window)
    assert gb.calls["Observe"] == 1 and gs.calls["Observe"] > 40


def test_batched_harness_writes_the_sequential_text_minopt(knobs, golden_dir):
    text = _golden(golden_dir, "barebones.csv")
    make = lambda: BatchOracleGP(1, SIMIL, NOISE)  # noqa: E731
    _same_text(make, text, 3, SEED=8, ITERS=20, MINOPT=6)
    _same_text(make, text, 3, SEED=9, MINOPT=100)  # no window optimised at all


def test_batched_harness_writes_the_sequential_text_hyperpriors(knobs, golden_dir):
    text = _golden(golden_dir, "hyperpriors.csv")
    make = lambda: BatchOracleGP(1, HYPER_SIMIL, kernel.ScaledNoise(0.01))  # noqa: E731
    seq, _, _ = _same_text(make, text, 6, model=lambda g: Model(g, priors.HyperPriors()), SEED=7, ITERS=15)
    assert len(seq.strip().split("\n")) == 44


def test_batched_harness_long_csv_falls_back_to_sequential_windows(knobs):
    rng = np.random.default_rng(0)
    n = 140
    x = np.arange(n) * 0.15
    y = np.sin(x) + 0.1 * rng.normal(size=n)
    text = "".join("%r,%r\n" % (float(a), float(b)) for a, b in zip(x, y))
    make = lambda: BatchOracleGP(1, SIMIL, NOISE)  # noqa: E731
    seq, gs, gb = _same_text(make, text, 3, SEED=5, ITERS=3, OUTOFSAMPLE=True)
    assert len(seq.strip().split("\n")) == n + n - 1
    # windows of 0 .. 128 rows in the batch, the 11 longer ones through the sequential code
    assert [nn for _, nn, _ in gb.members] == list(range(129))
    assert len(gb.X) == n - 1


def test_batch_knob_changes_nothing_elsewhere(knobs, golden_dir):
    text = _golden(golden_dir, "barebones.csv")
    make = lambda: BatchOracleGP(1, SIMIL, NOISE)  # noqa: E731
    for kn in (dict(ALG="adam", ITERS=3), dict(OPTINP=True, ITERS=2)):
        seq, _, _ = _run(make, text, 3, SEED=4, BATCH=False, **kn)
        bat, gb, _ = _run(make, text, 3, SEED=4, BATCH=True, **kn)
        assert bat == seq and gb.calls["set_batch"] == 0


# ---- optimize.lbfgs_lockstep against lbfgs run alone ---------------------------------------------------------------
class Bowl:
    """A smooth objective with its own parameters (Observe: the value maximised, Gradient: its gradient); outside
    radius `wall` the point is 'not positive definite'."""

    def __init__(self, c, a, wall=np.inf):
        self.c, self.a, self.wall = np.asarray(c, float), np.asarray(a, float), wall
        self._x = None

    def Observe(self, x):
        x = np.asarray(x, dtype=float)
        if np.linalg.norm(x) > self.wall:
            raise NotPositiveDefinite(-1)
        self._x = x
        d = x - self.c
        return float(-(self.a * d * d).sum() - 0.1 * np.cos(3.0 * x).sum() - 0.05 * (d ** 4).sum())

    def Gradient(self):
        x = self._x
        d = x - self.c
        return -2.0 * self.a * d + 0.3 * np.sin(3.0 * x) - 0.2 * d ** 3


def test_lbfgs_lockstep_takes_the_path_of_lbfgs_alone():
    rng = np.random.default_rng(1)
    P = 4
    bowls = [Bowl(rng.normal(size=P), rng.uniform(0.2, 3.0, P)) for _ in range(6)]
    bowls.append(Bowl(np.zeros(P), np.ones(P), wall=0.5))  # infeasible start
    x0s = rng.normal(size=(len(bowls), P)) * 2.0
    x0s[-1] = 3.0
    calls = []

    def evaluate(idx, xs):
        calls.append(len(idx))
        out = []
        for i, x in zip(idx, xs):
            try:
                v = bowls[i].Observe(x)
            except NotPositiveDefinite:
                out.append((np.inf, None))
                continue
            out.append((-v, -np.asarray(bowls[i].Gradient(), dtype=float)))
        return out

    got = optimize.lbfgs_lockstep(evaluate, x0s, major_iterations=50, gradient_threshold=1e-9)
    for i, b in enumerate(bowls):
        if i == len(bowls) - 1:
            with pytest.raises(ValueError, match=optimize.INFEASIBLE_START):
                optimize.lbfgs(b, x0s[i], major_iterations=50, gradient_threshold=1e-9)
            assert got[i] is None
            continue
        want = optimize.lbfgs(b, x0s[i], major_iterations=50, gradient_threshold=1e-9)
        r = got[i]
        assert r.x.tobytes() == want.x.tobytes()
        assert r.grad.tobytes() == want.grad.tobytes()
        assert (r.lml, r.iterations, r.evaluations, r.converged) == (want.lml, want.iterations, want.evaluations,
                                                                     want.converged)
        assert r.history == want.history
    assert calls[0] == len(bowls) and max(calls) == len(bowls)  # every live run in every round

