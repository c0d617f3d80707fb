"""Event discounts on the GPU (gogp_set_events; tutorial/events/kernel/kernel.go:14-44) against the numpy restatement
of tests/events_ref.py: the case study itself (N = 43, the one-launch path), the general path, bit-identity with the
kernels without events where no discount applies, the full Observe form, NDim > 1, fp32 gradients, the sharded
evaluation and the refusals."""
import io
import os

import numpy as np
import pytest

import events_ref as R
from gogp_amd import kernel
from gogp_amd import _lib

pytestmark = pytest.mark.gpu

SIMIL = kernel.Scaled(kernel.Matern52)
NOISE = kernel.ScaledNoise(0.01)  # tutorial/events/main.go:66-72
SELF = kernel.parse_events(R.SELFCHECK)
# 8 events for the general path: overlapping (0, 1), from == to (2), outside the data (7)
EV8 = [(-0.6, 0.4, 0.5), (-0.2, 0.9, 0.3), (0.25, 0.25, 0.7), (1.1, 1.6, 0.2), (1.3, 1.45, 0.9), (-1.5, -1.2, 0.4),
       (1.8, 2.9, 0.6), (5.0, 6.0, 0.05)]


def _data(golden_dir):
    d = np.loadtxt(os.path.join(golden_dir, "events.csv"), delimiter=",")
    return d[:, :1].copy(), (d[:, 1] - d[:, 1].mean()) / d[:, 1].std(ddof=1)


def _synth(n, D=1, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (n, D))
    y = np.sin(2.0 * X[:, 0]) + 0.3 * X.sum(1) + 0.1 * rng.normal(size=n)
    return X, y


def _gp(D, events, X, y, axis=0, **kw):
    from gogp_amd.gp import GP
    simil = kernel.Events(SIMIL, events, axis) if events is not None else SIMIL
    return GP(D, simil, NOISE, X=X, Y=y, device=0, **kw)


def _ref(D, events, X, y, axis=0):
    r = R.RefGP(D, events, axis)
    r.X, r.Y = X, y
    return r


def _check(g, r, x, Zs, lml_tol=1e-10, grad_tol=1e-8, mu_tol=1e-9):
    lml, lml_r = g.Observe(x), r.Observe(x)
    assert abs(lml - lml_r) <= lml_tol * abs(lml_r), (lml, lml_r)
    gr, gr_r = g.Gradient(), r.Gradient()
    np.testing.assert_allclose(gr, gr_r, rtol=grad_tol, atol=grad_tol * np.abs(gr_r).max())
    np.testing.assert_allclose(g.Alpha, r.alpha, rtol=1e-8, atol=1e-8 * np.abs(r.alpha).max())
    for Z in Zs:
        mu, sg = g.Produce(Z)
        mu_r, sg_r = r.Produce(Z)
        np.testing.assert_allclose(mu, mu_r, rtol=mu_tol, atol=mu_tol * max(1.0, np.abs(mu_r).max()))
        np.testing.assert_allclose(sg, sg_r, rtol=1e-7, atol=1e-8)


def test_case_study_matches_the_restatement(golden_dir):
    """events.csv (N = 43, the tiny one-launch path), the selfcheck events, several theta; Produce at M = 1, 16, 64 and at
    points exactly on the boundaries 1.0 and 6.7 (x = 6.7 is also a data point: the inclusive to <= xb case)."""
    X, y = _data(golden_dir)
    assert len(y) == 43 and np.any(X[:, 0] == 6.7)
    g, r = _gp(1, SELF, X, y), _ref(1, SELF, X, y)
    rng = np.random.default_rng(1)
    Zs = [np.array([[3.3]]), rng.uniform(0, 9, (16, 1)), rng.uniform(0, 9, (64, 1)),
          np.array([[1.0], [6.7], [4.2], [0.9999], [6.7001]])]
    for th in ([1.0, 1.0, 1.0], [2.3, 0.4, 0.3], [0.6, 2.5, 1.7]):
        _check(g, r, np.log(th), Zs)
    # the discount changes the answer: the same data without events do not match the restatement
    plain = _gp(1, None, X, y)
    x = np.log([2.3, 0.4, 0.3])
    assert abs(plain.Observe(x) - r.Observe(x)) > 1e-3
    g.close()
    plain.close()


def _evaluate(golden_dir, **knobs):
    """Evaluate(gp, gp, theta, ...) as tutorial/events/main.go:65-76 on the GPU GP and on the restatement."""
    from gogp_amd import tutorial
    from gogp_amd.gp import GP
    saved = {k: getattr(tutorial, k) for k in knobs}
    try:
        for k, v in knobs.items():
            setattr(tutorial, k, v)
        outs = []
        for gp in (GP(1, kernel.Events(SIMIL, SELF), NOISE, device=0), R.RefGP(1, SELF)):
            out = io.StringIO()
            with open(os.path.join(golden_dir, "events.csv")) as f:
                tutorial.Evaluate(gp, gp, np.zeros(3), f, out, log=io.StringIO())
            outs.append([[float(v) for v in ln.split(",")] for ln in out.getvalue().strip().split("\n")])
    finally:
        for k, v in saved.items():
            setattr(tutorial, k, v)
    got, want = outs
    assert len(got) == len(want) > 30
    return got, want


def test_case_study_through_the_tutorial_harness(golden_dir):
    """Without optimisation (MINOPT above N) every row is an Observe + Produce: the same text as the restatement."""
    got, want = _evaluate(golden_dir, MINOPT=100, OUTOFSAMPLE=True, SEED=7)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6)  # %f: 6 decimals


def test_case_study_optimised_through_the_tutorial_harness(golden_dir):
    """The case study as it runs: L-BFGS fits the hyperparameters on the points before each row once there are more
    than MINOPT of them (tutorial/tutorial.go:128-155), then forecasts.  Same seed on the GPU GP and on the restatement:
    the same final LML and forecast mean (L-BFGS follows the same path while LML and gradient agree to ~1e-13; the
    tolerance allows for late divergence of the iterates, as tests/test_tutorial.py does)."""
    got, want = _evaluate(golden_dir, MINOPT=30, ITERS=30, SEED=12)
    optimised = 0
    for g, w in zip(got, want):
        assert abs(g[5] - w[5]) <= 1e-3 * max(1.0, abs(w[5])), (g, w)   # final LML
        assert abs(g[2] - w[2]) <= 1e-3 * max(1.0, abs(w[2])), (g, w)   # forecast mean
        optimised += g[4] != g[5]  # initial and final LML differ where the optimiser ran
    assert optimised >= 5


@pytest.mark.parametrize("n", [1500, 4096])
def test_general_path_matches_the_restatement(n):
    X, y = _synth(n)
    g, r = _gp(1, EV8, X, y), _ref(1, EV8, X, y)
    rng = np.random.default_rng(2)
    Zs = [rng.uniform(-2, 2, (1, 1)), rng.uniform(-2, 2, (16, 1)), rng.uniform(-2.5, 2.5, (64, 1)),
          np.array([[0.25], [0.4], [-0.6], [1.6]]), rng.uniform(-2, 2, (300, 1))]
    for th in ([1.0, 0.7, 0.5], [2.0, 0.3, 0.2]):
        _check(g, r, np.log(th), Zs, lml_tol=1e-10 if n < 4096 else 1e-9)
    # candidates (k = 8): bit-equal to 8 single calls
    xs = np.log(np.array([[1.0 + 0.1 * i, 0.5 + 0.05 * i, 0.3 + 0.02 * i] for i in range(8)]))
    lml_k, grad_k, st = g.observe_gradient_candidates(xs)
    assert (st == 0).all()
    for i in range(8):
        assert g.Observe(xs[i]) == lml_k[i]
        np.testing.assert_array_equal(g.Gradient(), grad_k[i])
    g.close()


def _outputs(g, x, Z):
    lml = g.Observe(x)
    return lml, g.Gradient(), *g.Produce(Z)


@pytest.mark.parametrize("n", [43, 700])
def test_bit_identity_where_no_discount_applies(n):
    """Discounts of 1.0; boundaries outside all data and test points; events set, then cleared: every bit of LML,
    gradient, mu and sigma equals the handle that never had events (tiny path at n = 43, the general path at 700)."""
    X, y = _synth(n, seed=9)
    Z = np.random.default_rng(4).uniform(-2, 2, (40, 1))
    x = np.log([1.4, 0.6, 0.4])
    want = _outputs(_gp(1, None, X, y), x, Z)
    cases = [[(-1.0, 0.5, 1.0), (0.1, 0.1, 1.0), (0.7, 1.9, 1.0)],
             [(5.0, 6.0, 0.5), (-9.0, -3.0, 0.25), (2.5, 2.5, 0.1)]]
    for ev in cases:
        got = _outputs(_gp(1, ev, X, y), x, Z)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    g = _gp(1, EV8, X, y)
    assert g.Observe(x) != want[0]
    L = _lib.lib()
    assert L.gogp_set_events(g._h, None, 0, 0) == _lib.GOGP_OK
    got = _outputs(g, x, Z)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("n", [40, 300])
def test_full_form_input_gradient(n):
    """The input gradient of the full Observe form against central differences of the LML (inputs kept >= 1e-3 away
    from every boundary, where the discount is constant)."""
    rng = np.random.default_rng(11)
    X = rng.uniform(-2, 2, n)
    bounds = np.array([b for e in EV8 for b in e[:2]])
    X = X[np.min(np.abs(X[:, None] - bounds[None, :]), axis=1) > 2e-3][:, None]
    y = np.sin(2.0 * X[:, 0])
    m = len(y)
    g = _gp(1, EV8, X, y)
    r = _ref(1, EV8, X, y)
    x = np.concatenate([np.log([1.2, 0.6, 0.4]), X.ravel(), y])
    lml = g.Observe(x)
    assert abs(lml - r.Observe(x)) <= 1e-10 * abs(lml)
    grad = g.Gradient()
    np.testing.assert_allclose(grad[:3], r.Gradient(), rtol=1e-8, atol=1e-8 * np.abs(grad[:3]).max())
    h = 1e-6
    for i in rng.choice(m, 12, replace=False):
        e = np.zeros_like(x)
        e[3 + i] = h
        fd = (r.Observe(x + e) - r.Observe(x - e)) / (2 * h)
        assert abs(grad[3 + i] - fd) <= 1e-5 * max(1.0, abs(fd)), (i, grad[3 + i], fd)
    g.close()


@pytest.mark.parametrize("n", [100, 900])
def test_three_dimensions_axis_one(n):
    rng = np.random.default_rng(12)
    X = rng.uniform(-1.5, 1.5, (n, 3))
    y = np.sin(X[:, 1]) + 0.5 * X[:, 0] - 0.2 * X[:, 2]
    ev = [(-0.5, 0.2, 0.4), (0.0, 0.0, 0.8), (0.6, 1.0, 0.3)]
    g, r = _gp(3, ev, X, y, axis=1), _ref(3, ev, X, y, axis=1)
    Z = rng.uniform(-1.5, 1.5, (20, 3))
    _check(g, r, np.log([1.1, 1.3, 0.5]), [Z])
    g.close()


def test_sixty_four_dimensions_axis_three():
    """GOGP_MAX_NDIM dimensions with events, beyond the one-launch path (N = 130): the Gram and cross launches ask for
    1024 D + 1024 = 66560 bytes of dynamic LDS there, more than 64 KB."""
    n, D = 130, 64
    rng = np.random.default_rng(13)
    X = rng.uniform(-1.5, 1.5, (n, D))
    y = np.sin(X[:, 3]) + 0.1 * X.sum(1)
    ev = [(-0.5, 0.2, 0.4), (0.6, 1.0, 0.3)]
    g, r = _gp(D, ev, X, y, axis=3), _ref(D, ev, X, y, axis=3)
    Z = rng.uniform(-1.5, 1.5, (20, D))
    _check(g, r, np.log([1.1, 8.0, 0.5]), [Z])
    g.close()


def _fp32_case():
    X, y = _synth(2500, seed=21)
    return X, y, np.log([1.0, 0.3, 3.0]), np.random.default_rng(3).uniform(-2, 2, (32, 1))


def _fp32_contract(lml, grad, alpha, mu, sg, ref):
    """The accuracy contract of the fp32 path against fp64 (tests/test_sharded.py, fp32 tiles)."""
    lml64, gr64, a64, mu64, sg64 = ref
    assert abs(lml - lml64) <= 2e-6 * abs(lml64), (lml, lml64)
    assert np.abs(grad - gr64).max() <= 2e-5 * np.abs(gr64).max(), (grad, gr64)
    assert np.abs(alpha - a64).max() <= 2e-5 * np.abs(a64).max()
    assert np.abs(mu - mu64).max() <= 1e-3 * np.abs(mu64).max()
    assert np.abs(sg - sg64).max() <= 2e-4 * np.abs(sg64).max()


def _fp64_events(X, y, x, Z):
    g = _gp(1, EV8, X, y)
    lml, grad = g.Observe(x), g.Gradient()
    alpha = g.Alpha.copy()
    mu, sg = g.Produce(Z)
    g.close()
    return lml, grad, alpha, mu, sg


def test_fp32_paths():
    """precision = 32 (the whole fp32 path: float Gram tiles, kmatvec_kernel_ev refinement, float K^-1 reduction) and
    gradient_precision = 32 (K^-1 on the fp32 tile kernel) with events, against the fp64 events result at the fixed
    tolerances of the fp32 contract."""
    X, y, x, Z = _fp32_case()
    ref = _fp64_events(X, y, x, Z)
    f32 = _gp(1, EV8, X, y, precision=32)
    lml, grad = f32.Observe(x), f32.Gradient()
    alpha = f32.Alpha.copy()
    mu, sg = f32.Produce(Z)
    _fp32_contract(lml, grad, alpha, mu, sg, ref)
    f32.close()
    mixed = _gp(1, EV8, X, y)
    mixed.set_option("gradient_precision", 32)
    assert mixed.Observe(x) == ref[0]  # Observe stays fp64
    assert np.abs(mixed.Gradient() - ref[1]).max() <= 2e-5 * np.abs(ref[1]).max()
    mixed.close()


@pytest.mark.parametrize("grid", [(1, 2), (2, 2)], ids=lambda g: "%dx%d" % g)
def test_sharded_fp32_with_events(grid):
    """Float shards with events (gram_local_kernel_ev<float>, the refinement's K alpha through kmatvec_kernel_ev over
    the ranks' column shares, grad_reduce_kernel_ev<0, true, float, *>): the fp32 contract against the fp64 events
    result, the same numbers on every rank."""
    from gogp_amd.sharded import ShardedGP
    import loopback
    X, y, x, Z = _fp32_case()
    ref = _fp64_events(X, y, x, Z)
    world = grid[0] * grid[1]

    def rank_fn(rk, lb):
        sh = ShardedGP(1, kernel.Events(SIMIL, EV8), NOISE, X=X, Y=y, device=0, precision=32, grid=grid, rank=rk,
                       world=world, exchange=lb.exchange, allreduce=lb.allreduce)
        lml, grad = sh.Observe(x), sh.Gradient()
        alpha = sh.Alpha.copy()
        mu, sg = sh.Produce(Z)
        sh.close()
        return lml, grad, alpha, mu, sg

    outs, lb = loopback.run_ranks(world, rank_fn)
    assert loopback.check_rendezvous(lb.log) is None
    for lml, grad, alpha, mu, sg in outs:
        _fp32_contract(lml, grad, alpha, mu, sg, ref)
        assert lml == outs[0][0] and np.array_equal(grad, outs[0][1])


def test_observe_gradient_batch_with_events():
    """gogp_observe_gradient_batch over handles with events (and one without): each equals its own Observe + Gradient."""
    from gogp_amd import gp as G
    X, y = _synth(900, seed=41)
    gps = [_gp(1, EV8, X[:700], y[:700]), _gp(1, SELF, 4.0 * X[:500] + 4.0, y[:500]), _gp(1, None, X[:600], y[:600])]
    xs = np.log([[1.1, 0.6, 0.4], [0.9, 0.8, 0.5], [1.3, 0.5, 0.3]])
    lmls, grads = G.observe_gradient_batch(gps, xs)
    for i, g in enumerate(gps):
        lml = g.Observe(xs[i])
        assert abs(lml - lmls[i]) <= 1e-12 * abs(lml)
        np.testing.assert_allclose(grads[i], g.Gradient(), rtol=1e-11, atol=1e-11 * np.abs(grads[i]).max())
    r = _ref(1, EV8, X[:700], y[:700])
    assert abs(lmls[0] - r.Observe(xs[0])) <= 1e-10 * abs(lmls[0])
    for g in gps:
        g.close()


def test_cpp_host_set_events(tmp_path):
    """gogp::GP::SetEvents (gogp_amd/host/gogp.hpp) refuses a vector that is not made of triples and discounts like the
    restatement."""
    import math
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_events_driver")
    libdir = os.path.join(root, "gogp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp_events_driver.cpp"), "-o", exe,
                           "-L" + libdir, "-lgogp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = np.array([float(v) for v in out.stdout.split()])
    X = (0.1 + 0.2 * np.arange(43))[:, None]
    r = _ref(1, SELF, X, np.sin(X[:, 0]))
    lml = r.Observe(np.log([1.5, 0.8, 0.6]))
    assert abs(vals[0] - lml) <= 1e-10 * abs(lml)
    np.testing.assert_allclose(vals[1:], r.Gradient(), rtol=1e-8, atol=1e-8 * np.abs(r.Gradient()).max())
    assert math.isfinite(vals[0])


@pytest.mark.parametrize("grid", [(1, 2), (2, 2)], ids=lambda g: "%dx%d" % g)
def test_sharded_matches_one_gpu(grid):
    from gogp_amd.sharded import ShardedGP
    import loopback
    world = grid[0] * grid[1]
    X, y = _synth(700, seed=31)
    x = np.log([1.3, 0.5, 0.4])
    Z = np.random.default_rng(6).uniform(-2, 2, (30, 1))
    one = _gp(1, EV8, X, y)
    lml1, g1 = one.Observe(x), one.Gradient()
    mu1, s1 = one.Produce(Z)
    one.close()

    def rank_fn(rk, lb):
        sh = ShardedGP(1, kernel.Events(SIMIL, EV8), NOISE, X=X, Y=y, device=0, grid=grid, rank=rk, world=world,
                       exchange=lb.exchange, allreduce=lb.allreduce)
        lml = sh.Observe(x)
        g = sh.Gradient()
        mu, s = sh.Produce(Z)
        sh.close()
        return lml, g, mu, s

    outs, _ = loopback.run_ranks(world, rank_fn)
    for lml, g, mu, s in outs:
        assert abs(lml - lml1) <= 1e-10 * abs(lml1), (lml, lml1)
        np.testing.assert_allclose(g, g1, rtol=1e-8, atol=1e-8 * np.abs(g1).max())
        np.testing.assert_allclose(mu, mu1, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(s, s1, rtol=1e-8, atol=1e-9)


def test_refusals():
    """Events with an ARD term are refused (GOGP_EARG with a message); so are bad arguments, on a live handle."""
    from gogp_amd.gp import GP, _dp
    L = _lib.lib()
    g = GP(2, kernel.Scaled(kernel.ARD(kernel.Matern52, 2)), NOISE, device=0)
    ev = np.array([[0.0, 1.0, 0.5]])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == _lib.GOGP_EARG
    assert b"ARD" in L.gogp_last_error(g._h)
    g.close()
    g = _gp(1, None, *_synth(50))
    assert L.gogp_set_events(g._h, _dp(ev), 1, 1) == _lib.GOGP_EARG  # axis >= ndim
    bad = np.array([[0.0, np.inf, 0.5]])
    assert L.gogp_set_events(g._h, _dp(bad), 1, 0) == _lib.GOGP_EARG
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == _lib.GOGP_OK
    g.close()
