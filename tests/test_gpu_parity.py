"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called
through the C ABI, against the CPU oracle and the reference's known answers.

Tolerances: north_star asks LML / mu / sigma within 1e-6 relative (fp64); the
reference's own tests use 1e-6 absolute (gp/gp_test.go:150,157,233) and 1e-4 for
gradient components (gp/gp_test.go:170,248).  We test 1e-6 absolute on the
known answers, <= 1e-8 relative on LML against the oracle, 1e-6 relative on
mu/sigma and 1e-6 relative (scaled by the gradient norm) on the gradient.
"""
import json
import math
import os

import numpy as np
import pytest

from gogp_amd import kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpmod():
    from gogp_amd import gp
    return gp


def _noise(spec):
    if spec["kind"] == "constant":
        return kernel.ConstantNoise(spec["std"])
    return kernel.UniformNoise


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "gp_test_known_answers.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# the tile kernel in isolation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 16), (256, 128, 64), (128, 384, 272), (512, 512, 256)])
def test_dgemm_tile_kernel(gpmod, M, N, K):
    rng = np.random.default_rng(M + N + K)
    A = rng.normal(size=(M, K))
    B = rng.normal(size=(N, K))
    C = rng.normal(size=(M, N))
    got = gpmod.dgemm_nt_check(A, B, C, alpha=-1.0, beta=1.0)
    want = C - A @ B.T
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * K)
    got = gpmod.dgemm_nt_check(A, B, C, alpha=1.0, beta=0.0)
    np.testing.assert_allclose(got, A @ B.T, rtol=0, atol=1e-12 * K)


def test_dgemm_fragment_layout_asymmetric(gpmod):
    """A = I against an asymmetric integer B catches a transposed C/D fragment
    map (f64 MFMA uses row = (lane>>4) + 4*reg, not the f32 map)."""
    M = N = K = 128
    A = np.eye(M, K)
    B = np.arange(N * K, dtype=float).reshape(N, K)  # B[n][k] = n*K + k
    got = gpmod.dgemm_nt_check(A, B, np.zeros((M, N)))
    np.testing.assert_array_equal(got, B.T)


# ---------------------------------------------------------------------------
# the reference's own known answers through the HIP path
# ---------------------------------------------------------------------------
def test_produce_known_answers(gpmod, known):
    # gp/gp_test.go:133-162
    for c in known["produce"]:
        for parallel in (False, True):
            g = gpmod.GP(1, kernel.Normal, _noise(c["noise"]), ThetaSimil=c["theta_simil"],
                         Parallel=parallel)
            g.Absorb(np.array(c["x"], dtype=float).reshape(-1, 1), c["y"])
            mu, sigma = g.Produce(c["z"])
            assert len(mu) == len(c["mu"]) and len(sigma) == len(c["sigma"])
            for got, want in zip(mu, c["mu"]):
                assert abs(got - want) <= 1e-6, (c["name"], mu)
            for got, want in zip(sigma, c["sigma"]):
                if math.isnan(got):  # the reference lets NaN pass
                    assert want == 0
                    continue
                # sigma = sqrt(variance - covariance) with variance ~ covariance:
                # sqrt amplifies 1e-16 rounding to 1e-8
                assert abs(got - want) <= 1e-6, (c["name"], sigma)


def test_elemental_model_known_answers(gpmod, known):
    # gp/gp_test.go:231-267
    from oracle.oracle import Oracle
    for c in known["elemental"]:
        x = np.array(c["x"], dtype=float)
        g = gpmod.GP(1, kernel.Normal, _noise(c["noise"]))
        ll = g.Observe(x)  # full form: inputs and outputs carried in x
        assert abs(ll - c["ll"]) < 1e-6, c["name"]
        dll = g.Gradient()
        assert len(dll) == len(x)  # gp_test.go:237
        # every component against a forward difference, as gp_test.go:242-252
        dx, eps = known["fd"]["dx"], known["fd"]["eps"]
        for j in range(len(x)):
            xj = x.copy()
            xj[j] += dx
            assert abs(dll[j] - (g.Observe(xj) - ll) / dx) <= eps, (c["name"], j)
        P = g._ns + g._nn
        n = (len(x) - P) // 2
        # hyperparameters-only form (gp_test.go:254-267)
        g2 = gpmod.GP(1, kernel.Normal, _noise(c["noise"]), X=x[P:P + n].reshape(-1, 1),
                      Y=x[P + n:])
        ll2 = g2.Observe(x[:P])
        dll2 = g2.Gradient()
        assert abs(ll2 - c["ll"]) < 1e-6
        assert len(dll2) == P
        o = Oracle(1, kernel.Normal, _noise(c["noise"]))
        o.set_data(x[P:P + n].reshape(-1, 1), x[P + n:])
        o.Observe(x[:P])
        np.testing.assert_allclose(dll2, o.Gradient(), rtol=1e-8, atol=1e-10)


# ---------------------------------------------------------------------------
# HIP path vs oracle on seeded inputs
# ---------------------------------------------------------------------------
def _data(rng, n, D):
    X = rng.uniform(0, 1, (n, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=n)
    if n > 1:
        y = (y - y.mean()) / y.std()
    return X, y


from cases import CASES  # noqa: E402  (shared with tests/golden/make_oracle_vectors.py)


def _check_against(gpmod, oracle_cls, name, D, simil, noise, ts, tn, n, m, seed,
                   lml_rtol=1e-8, grad_rtol=1e-6):
    rng = np.random.default_rng(seed)
    X, y = _data(rng, n, D)
    Z = rng.uniform(-0.1, 1.1, (m, D))
    x = np.log(np.array(list(ts) + list(tn)))
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    o = oracle_cls(D, simil, noise)
    o.set_data(X, y)
    lml, lml_o = g.Observe(x), o.Observe(x)
    assert abs(lml - lml_o) <= lml_rtol * max(1.0, abs(lml_o)), (name, lml, lml_o)
    grad, grad_o = g.Gradient(), o.Gradient()
    scale = max(1.0, np.abs(grad_o).max())
    assert np.abs(grad - grad_o).max() <= grad_rtol * scale, (name, grad, grad_o)
    mu, sigma = g.Produce(Z)
    mu_o, sigma_o = o.Produce(Z)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=name)
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8, err_msg=name)
    # cached state: gp.GP.Alpha / gp.GP.L (gp/gp.go:35-36)
    alpha_o = o.Alpha
    np.testing.assert_allclose(g.Alpha, alpha_o, rtol=1e-6, atol=1e-8 * np.abs(alpha_o).max())
    return g, o


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", CASES, ids=[c[0] for c in CASES])
def test_small_vs_faithful_oracle(gpmod, name, D, simil, noise, ts, tn):
    from oracle.oracle import Oracle
    g, o = _check_against(gpmod, Oracle, name, D, simil, noise, ts, tn, n=50, m=9, seed=7)
    np.testing.assert_allclose(g.L, o.L, rtol=1e-8, atol=1e-10)


def test_oracle_vectors(gpmod, golden_dir):
    """HIP path against the committed oracle regression vectors (every kernel family
    at N in {2, 20, 64, 256, 1024}; tests/golden/make_oracle_vectors.py)."""
    from gogp_amd import synth
    with open(os.path.join(golden_dir, "oracle_vectors.json")) as f:
        vectors = json.load(f)["vectors"]
    cases = {c[0]: c for c in CASES}
    assert len(vectors) == 5 * len(CASES)
    for v in vectors:
        _, D, simil, noise, _, _ = cases[v["case"]]
        X, y = synth.make_inputs(v["n"], D, v["seed"])
        Z = synth.make_test_points(v["m"], D, v["seed"] + 1)
        assert X.sum() == v["x_sum"] and y.sum() == v["y_sum"] and Z.sum() == v["z_sum"]
        g = gpmod.GP(D, simil, noise, X=X, Y=y)
        tag = (v["case"], v["n"])
        lml = g.Observe(np.array(v["log_theta"]))
        assert abs(lml - v["lml"]) <= 1e-8 * max(1.0, abs(v["lml"])), (tag, lml, v["lml"])
        grad, want = g.Gradient(), np.array(v["grad"])
        assert np.abs(grad - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (tag, grad, want)
        mu, sigma = g.Produce(Z)
        np.testing.assert_allclose(mu, v["mu"], rtol=1e-6, atol=1e-7, err_msg=str(tag))
        np.testing.assert_allclose(sigma, v["sigma"], rtol=1e-6, atol=1e-6, err_msg=str(tag))
        g.close()


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 255, 256, 257, 700])
def test_ragged_sizes(gpmod, n):
    """Padding edges: N below / at / above the 128 tile and 256 panel sizes."""
    from oracle.oracle import FastOracle
    _check_against(gpmod, FastOracle, "n=%d" % n, 3, kernel.Scaled(kernel.Normal),
                   kernel.UniformNoise, [1.0, 0.6], [0.2], n=n, m=5, seed=100 + n)


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", CASES[:6], ids=[c[0] for c in CASES[:6]])
def test_mid_vs_fast_oracle(gpmod, name, D, simil, noise, ts, tn):
    from oracle.oracle import FastOracle
    _check_against(gpmod, FastOracle, name, D, simil, noise, ts, tn, n=1500, m=200, seed=11)


def test_config2_n4096_d4(gpmod):
    """BASELINE config 2: RBF + homoscedastic noise, N=4096, D=4, fp64."""
    from oracle.oracle import FastOracle
    D = 4
    _check_against(gpmod, FastOracle, "config2", D, kernel.Scaled(kernel.Normal), kernel.UniformNoise,
                   [1.0, math.sqrt(D / 6.0)], [0.1], n=4096, m=256, seed=20251115)


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", [c for c in CASES if c[0] in (
    "scaled_rbf", "ard_rbf", "matern32", "matern52_ref", "periodic", "hyperpriors")],
    ids=lambda v: v if isinstance(v, str) else None)
def test_full_form_gradient_vs_faithful_oracle(gpmod, name, D, simil, noise, ts, tn):
    """Observe with inputs and outputs carried in x (gp/gp.go:366-369): gradient
    w.r.t. hyperparameters, every input coordinate and every output
    (gp/gp.go:118-129,488-493) against the faithful oracle's dense-dK gradient."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(17)
    n = 37
    X, y = _data(rng, n, D)
    x = np.concatenate([np.log(np.array(list(ts) + list(tn))), X.reshape(-1), y])
    g = gpmod.GP(D, simil, noise)
    o = Oracle(D, simil, noise)
    lml, lml_o = g.Observe(x), o.Observe(x)
    assert abs(lml - lml_o) <= 1e-8 * max(1.0, abs(lml_o))
    grad, grad_o = g.Gradient(), o.Gradient()
    assert grad.shape == grad_o.shape == x.shape
    scale = max(1.0, np.abs(grad_o).max())
    assert np.abs(grad - grad_o).max() <= 1e-6 * scale, (name, np.abs(grad - grad_o).argmax())
    np.testing.assert_array_equal(g.X, X)  # gp/gp.go:391-396: X, Y re-sliced from x
    np.testing.assert_array_equal(g.Y, y)


@pytest.mark.parametrize("D", [40, 64])
def test_full_form_gradient_at_max_ndim(gpmod, D):
    """NDim up to GOGP_MAX_NDIM = 64: the input-gradient kernel needs 99 KB of dynamic LDS at
    D = 64 (above the 64 KB default limit, raised explicitly); hyperparameters-only and full
    forms with an ARD kernel against the faithful oracle."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(D)
    n = 70
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.UniformNoise
    th = np.concatenate([[1.1], np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)), [0.2]])
    x = np.concatenate([np.log(th), X.reshape(-1), y])
    g = gpmod.GP(D, simil, noise)
    o = Oracle(D, simil, noise)
    lml, lml_o = g.Observe(x), o.Observe(x)
    assert abs(lml - lml_o) <= 1e-8 * max(1.0, abs(lml_o))
    grad, grad_o = g.Gradient(), o.Gradient()
    assert grad.shape == grad_o.shape == x.shape
    assert np.abs(grad - grad_o).max() <= 1e-6 * max(1.0, np.abs(grad_o).max())
    g2 = gpmod.GP(D, simil, noise, X=X, Y=y)
    assert abs(g2.Observe(np.log(th)) - lml_o) <= 1e-8 * max(1.0, abs(lml_o))
    np.testing.assert_allclose(g2.Gradient(), grad_o[:D + 2], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("D,n", [(24, 900), (40, 4200)])
def test_ard_gradient_many_dimensions_two_terms(gpmod, D, n):
    """The same with a second term (ARD-RBF + Matern-3/2): multi-term kernels take the per-pair
    instances of the reduction (passes of 16 ARD dimensions), single-term ones the restructured
    instances below."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(200 + D)
    X, y = _data(rng, n, D)
    simil = kernel.Sum([kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.Scaled(kernel.Matern32)])
    noise = kernel.UniformNoise
    th = np.concatenate([[1.1], np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)), [0.3, 1.5], [0.2]])
    assert simil.NTheta() + 1 == th.size
    x = np.log(th)
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    assert abs(g.Observe(x) - lml_o) <= 1e-9 * abs(lml_o)
    g1 = g.Gradient()
    g.Observe(x)
    np.testing.assert_array_equal(g1, g.Gradient())
    assert np.abs(g1 - grad_o).max() <= 1e-7 * max(1.0, np.abs(grad_o).max())
    g.close()


@pytest.mark.parametrize("kind", ["normal", "matern52"])
@pytest.mark.parametrize("D,n", [(2, 700), (9, 900), (12, 900), (16, 2300), (17, 900), (24, 900), (32, 900), (33, 900), (40, 4200),
                                 (48, 700), (49, 1300), (64, 4200)])
def test_ard_gradient_many_dimensions(gpmod, D, n, kind):
    """ARD kernels with one radial term take grad_mfma.hip: distances and the per-dimension sums on the
    matrix cores (S = Xs Xs^T and P = G Xs per 64x64 tile), every D padded to a multiple of 16 (option
    ard_mfma_min_dims = 65 selects the scalar-row kernel of grad.hip instead: second half of the test).
    n = 4200 gives every workgroup
    several tiles, D = 16 / 32 / 48 / 64 are the exact pad sizes, 17 / 33 / 49 one past them.  Against the
    oracle, and bit-for-bit repeatable."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(100 + D)
    X, y = _data(rng, n, D)
    base = kernel.Normal if kind == "normal" else kernel.Matern52
    simil, noise = kernel.Scaled(kernel.ARD(base, D)), kernel.UniformNoise
    th = np.concatenate([[1.1], np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)), [0.2]])
    x = np.log(th)
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    grads = []
    for _ in range(3):
        assert abs(g.Observe(x) - lml_o) <= 1e-9 * abs(lml_o)
        grads.append(g.Gradient())
    np.testing.assert_array_equal(grads[0], grads[1])
    np.testing.assert_array_equal(grads[0], grads[2])
    assert np.abs(grads[0] - grad_o).max() <= 1e-7 * max(1.0, np.abs(grad_o).max())
    g.set_option("ard_mfma_min_dims", 65)  # the scalar-row instances of grad.hip on the same data
    g.Observe(x)
    assert np.abs(g.Gradient() - grad_o).max() <= 1e-7 * max(1.0, np.abs(grad_o).max())
    g.close()


@pytest.mark.parametrize("D,n", [(3, 900), (20, 1500)])
def test_ard_gradient_offset_inputs(gpmod, D, n):
    """Uncentred inputs (timestamps): every coordinate carries an offset of 1e6 length scales.  The reference and
    the oracle work on per-pair differences; the matrix-core reduction (grad_mfma.hip) expands r^2 = |a|^2 + |b|^2
    - 2 a.b and must therefore centre each tile first -- uncentred it loses eps * |x/l|^2 / u^2 ~ 1e-4.  The same
    problem without the offset is the reference value (the kernel is translation invariant)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(4242 + D)
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.UniformNoise
    ell = np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D))
    x = np.log(np.concatenate([[1.1], ell, [0.2]]))
    # power-of-two offsets keep X + off - off == X bit for bit where |X| < 1: both problems hold the SAME points
    off = 2.0 ** 20 * np.ones(D)
    assert off.min() / ell.max() > 2e5
    Xo = X + off
    X0 = Xo - off  # what survives the offset's rounding: the points the shifted problem really contains
    o = FastOracle(D, simil, noise)
    o.set_data(X0, y)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    g = gpmod.GP(D, simil, noise, X=Xo, Y=y)
    assert abs(g.Observe(x) - lml_o) <= 1e-9 * abs(lml_o)
    assert np.abs(g.Gradient() - grad_o).max() <= 1e-7 * max(1.0, np.abs(grad_o).max())
    g.set_option("ard_mfma_min_dims", 65)  # scalar-row kernel of grad.hip: per-pair differences, no expansion
    g.Observe(x)
    assert np.abs(g.Gradient() - grad_o).max() <= 1e-7 * max(1.0, np.abs(grad_o).max())
    g.close()


def test_full_form_gradient_mid_size(gpmod):
    """Input/output gradient at a size that spans several 64-row tiles and 256-panels,
    against central differences of the HIP LML itself on a few coordinates."""
    rng = np.random.default_rng(23)
    n, D = 300, 3
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
    x = np.concatenate([np.log([1.1, 0.6, 0.2]), X.reshape(-1), y])
    g = gpmod.GP(D, simil, noise)
    g.Observe(x)
    grad = g.Gradient()
    np.testing.assert_allclose(grad[3 + n * D:], -g.Alpha, rtol=1e-12, atol=1e-14)
    for j in [0, 1, 2, 3, 3 + 5, 3 + n * D - 1, 3 + 137 * D + 1, 3 + n * D + 7]:
        h = 1e-6
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd = (g.Observe(xp) - g.Observe(xm)) / (2 * h)
        assert abs(fd - grad[j]) <= 1e-5 * max(1.0, abs(fd)), (j, fd, grad[j])


def test_absorb_then_produce_and_restore(gpmod):
    """Absorb (no gradient) -> Produce; then 'Produce on stored results'
    (gp/gp.go:255-257) from exported L / Alpha."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(5)
    D, n = 2, 300
    X, y = _data(rng, n, D)
    Z = rng.uniform(0, 1, (33, D))
    simil, noise = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
    g = gpmod.GP(D, simil, noise, ThetaSimil=[1.1, 0.4], ThetaNoise=[0.2])
    g.Absorb(X, y)
    o = FastOracle(D, simil, noise)
    o.Absorb(X, y, [1.1, 0.4], [0.2])
    assert abs(g.LML() - o.LML()) <= 1e-8 * abs(o.LML())
    mu, sigma = g.Produce(Z)
    mu_o, sigma_o = o.Produce(Z)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8)
    with pytest.raises(gpmod.GogpError):
        g.Gradient()  # no Observe: the reference has no dK after Absorb either
    L, alpha = g.L, g.Alpha
    g2 = gpmod.GP(D, simil, noise, ThetaSimil=[1.1, 0.4], ThetaNoise=[0.2], X=X, Y=y)
    g2.restore(L, alpha)
    mu2, sigma2 = g2.Produce(Z)
    np.testing.assert_allclose(mu2, mu, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(sigma2, sigma, rtol=1e-9, atol=1e-12)
    assert abs(g2.LML() - g.LML()) <= 1e-9 * abs(g.LML())


@pytest.mark.parametrize("n,m", [(1, 1), (2, 3), (300, 1), (700, 1), (1500, 17), (2300, 33), (4096, 64), (5000, 5), (8192, 1)])
def test_produce_few_points_in_one_pass_over_the_factor(gpmod, n, m):
    """Produce for M <= 64 test points (the reference's harness asks for ONE per step, tutorial/tutorial.go:178-179;
    gp/gp.go:322-357): blocked forward substitution with the 256-block inverses in ONE persistent launch whose
    workgroups hand v_j / w_B to each other through counters in global memory (trsm_small.hip).  Against the oracle
    and against the tile-kernel route on the same factor -- right behind an eager Observe (the triangular inverse of
    the gradient still occupies the GPU: uneven load, workgroups not all resident at once), after an Absorb, after a
    Gradient, and on a restored factor; repeated calls agree bit for bit (fixed summation order)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(n * 100 + m)
    D = 3
    X, y = _data(rng, n, D)
    Z = rng.uniform(-0.1, 1.1, (m, D))
    simil, noise = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
    x = np.log([1.3, 0.6, 0.15])
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    g.Observe(x)
    mu1, s1 = g.Produce(Z)            # the inverse of the eager sweep is still running
    g.Gradient()
    mu2, s2 = g.Produce(Z)            # idle GPU
    np.testing.assert_array_equal(mu1, mu2)
    np.testing.assert_array_equal(s1, s2)
    g.set_option("produce_small_max", 0)
    mu0, s0 = g.Produce(Z)            # the tile-kernel route on the same factor
    g.set_option("produce_small_max", 64)
    np.testing.assert_allclose(mu1, mu0, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(s1, s0, rtol=1e-9, atol=1e-11)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    o.Observe(x)
    mu_o, s_o = o.Produce(Z)
    np.testing.assert_allclose(mu1, mu_o, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(s1, s_o, rtol=1e-6, atol=1e-8)
    # a new factor by Absorb (no gradient preparation), then the same state restored into another handle
    th = np.exp(np.log([0.9, 0.45, 0.2]))
    g3 = gpmod.GP(D, simil, noise, ThetaSimil=th[:2], ThetaNoise=th[2:], X=X, Y=y)
    g3.Absorb(X, y)
    mu3, s3 = g3.Produce(Z)
    o.Observe(np.log(th))
    mu_o3, s_o3 = o.Produce(Z)
    np.testing.assert_allclose(mu3, mu_o3, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(s3, s_o3, rtol=1e-6, atol=1e-8)
    g4 = gpmod.GP(D, simil, noise, ThetaSimil=th[:2], ThetaNoise=th[2:], X=X, Y=y)
    g4.restore(g3.L, g3.Alpha)
    mu4, s4 = g4.Produce(Z)
    np.testing.assert_allclose(mu4, mu3, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(s4, s3, rtol=1e-9, atol=1e-12)
    for h in (g, g3, g4):
        h.close()


@pytest.mark.parametrize("n,m,prec", [(700, 33, 64), (2300, 300, 64), (5000, 1100, 64), (2300, 300, 32)])
def test_produce_through_superpanel_inverses_matches_panel_substitution(gpmod, n, m, prec):
    """Produce solves V^T = Kstar^T L^-T super-panel by super-panel through T^-1, the inverse of the factor's diagonal
    block assembled from the 256-block inverses by the first Produce on a factor (api.hip: assemble_tinv; the batched
    plain products of solve.hip: blockmm_kernel) -- one product per super-panel instead of a solve + update per 256
    columns (gp/gp.go:337-342 is one SolveTo either way).  Against round 3's panel-by-panel substitution (option
    produce_tinv = 0) and the oracle; a second Produce reuses the inverses, another blocking (produce_panels) and a new
    factor rebuild them."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(n + m)
    D = 3
    X, y = _data(rng, n, D)
    Z = rng.uniform(-0.1, 1.1, (m, D))
    simil, noise = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
    x = np.log([1.3, 0.6, 0.15])
    g = gpmod.GP(D, simil, noise, X=X, Y=y, precision=prec)
    g.set_option("produce_small_max", 0)  # this test is about the tile-kernel route, whatever m (the one-pass kernel: below)
    g.Observe(x)
    mu1, s1 = g.Produce(Z)           # assembles T^-1
    mu2, s2 = g.Produce(Z)           # reuses it
    np.testing.assert_array_equal(mu1, mu2)
    np.testing.assert_array_equal(s1, s2)
    g.set_option("produce_tinv", 0)  # round 3's substitution on the same factor
    mu0, s0 = g.Produce(Z)
    tol = 1e-9 if prec == 64 else 2e-3
    np.testing.assert_allclose(mu1, mu0, rtol=tol, atol=tol)
    np.testing.assert_allclose(s1, s0, rtol=tol, atol=tol)
    g.set_option("produce_tinv", 1)
    for pw, groups in ((1, 1), (3, 4), (8, 2)):
        g.set_option("produce_panels", pw)
        g.set_option("produce_groups", groups)
        mu3, s3 = g.Produce(Z)
        np.testing.assert_allclose(mu3, mu0, rtol=tol, atol=tol)
        np.testing.assert_allclose(s3, s0, rtol=tol, atol=tol)
    if prec == 64:
        o = FastOracle(D, simil, noise)
        o.set_data(X, y)
        o.Observe(x)
        mu_o, s_o = o.Produce(Z)
        np.testing.assert_allclose(mu1, mu_o, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(s1, s_o, rtol=1e-6, atol=1e-8)
        x2 = np.log([0.9, 0.45, 0.2])  # a new factor: the inverses of the old one must not be used
        g.Observe(x2)
        o.Observe(x2)
        mu4, s4 = g.Produce(Z)
        mu_o, s_o = o.Produce(Z)
        np.testing.assert_allclose(mu4, mu_o, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(s4, s_o, rtol=1e-6, atol=1e-8)
    g.close()


def test_kinv_in_two_launches_is_bit_identical(gpmod):
    """Above the sizes whose K^-1 accumulates inside the sweep (npad > 10240) the first 60 % of the columns' part of
    K^-1 = Y Y^T is launched during the sweep and Gradient's launch adds the rest (api.hip: option kinv_split): the
    same sums in the same order.  Also: a factorisation whose early launch no Gradient picks up must not disturb the
    next one."""
    rng = np.random.default_rng(77)
    n, D = 10400, 3
    X, y = _data(rng, n, D)
    x = np.log([1.1, 0.6, 0.1])
    g = gpmod.GP(D, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, X=X, Y=y)
    g.set_option("kinv_split", 0)
    g.Observe(x)
    lml0, g0 = g.LML(), g.Gradient().copy()
    for pct in (60, 30, 90):
        g.set_option("kinv_split", pct)
        g.Observe(x)
        assert g.LML() == lml0
        np.testing.assert_array_equal(g.Gradient(), g0)
    g.Observe(x + 0.1)   # nobody asks for this gradient
    g.Observe(x)
    np.testing.assert_array_equal(g.Gradient(), g0)
    g.close()


@pytest.mark.parametrize("rows_below", [0, 64, 192, 1024])
def test_chain_step_kernel_against_numpy(rows_below):
    """panel128.hip alone (gp/gp.go:228, the diagonal-block factorisation and the panel solve of Factorize): the factor of
    a 128 x 128 block and the rows under it solved against it, against numpy's Cholesky / triangular solve."""
    import ctypes
    from gogp_amd import _lib
    H = _lib.hooks()
    rng = np.random.default_rng(rows_below + 1)
    n = 128 + rows_below
    B = rng.normal(size=(n, 150))
    K = B @ B.T / 150 + 0.3 * np.eye(n)
    A = np.ascontiguousarray(K[:, :128])
    L = np.zeros_like(A)
    st = (ctypes.c_uint64 * 72)()
    us = ctypes.c_double()
    assert H.gogp_test_panel128(0, A.ctypes.data_as(_lib._dp), L.ctypes.data_as(_lib._dp), rows_below, 1, st,
                                ctypes.byref(us)) == 0
    Ld = np.linalg.cholesky(K[:128, :128])
    np.testing.assert_allclose(L[:128], Ld, rtol=0, atol=1e-13 * np.abs(Ld).max())   # upper triangle: zeros
    if rows_below:
        ref = np.linalg.solve(Ld, K[128:, :128].T).T
        np.testing.assert_allclose(L[128:], ref, rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("rows_below", [64, 192, 1024])
def test_chain_step_result_does_not_depend_on_slabs_per_workgroup(rows_below):
    """panel128.hip, multi-slab workgroups (launches with more workgroups than compute units: k candidates, tall panels): a
    workgroup factors the diagonal block once and treats further slabs of 64 panel rows with the saved pivot scalings --
    the same operations on every row as the one-slab form, so the bits must agree whatever the number of slabs; candidates
    and single calls (gp/gp.go:228 behind both) stay bit-identical because of it."""
    import ctypes
    from gogp_amd import _lib
    H = _lib.hooks()
    rng = np.random.default_rng(rows_below + 7)
    n = 128 + rows_below
    B = rng.normal(size=(n, 150))
    K = B @ B.T / 150 + 0.3 * np.eye(n)
    A = np.ascontiguousarray(K[:, :128])
    outs = []
    for slabs in (1, 2, 3, 4):
        L = np.zeros_like(A)
        us = ctypes.c_double()
        assert H.gogp_test_panel128_slabs(0, A.ctypes.data_as(_lib._dp), L.ctypes.data_as(_lib._dp), rows_below, slabs, 1,
                                          ctypes.byref(us)) == 0
        outs.append(L)
    Ld = np.linalg.cholesky(K[:128, :128])
    ref = np.linalg.solve(Ld, K[128:, :128].T).T
    np.testing.assert_allclose(outs[0][128:], ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    for L in outs[1:]:
        np.testing.assert_array_equal(L, outs[0])


@pytest.mark.parametrize("name,D,simil,noise,ts,tn", CASES, ids=[c[0] for c in CASES])
def test_tutorial_sized_evaluations_in_one_launch(gpmod, name, D, simil, noise, ts, tn):
    """Option tiny (default on; gp/gp.go:89-239 at the reference's own sizes -- its case studies fit 20 .. 44 observations):
    for N <= 128 the Gram matrix, the factor, the block inverse, z, alpha and K^-1 come from ONE launch of one workgroup
    (diag256.hip: tiny_eval_kernel) instead of the general sweep's ~15 dependent launches.  Same numbers as the general sweep
    -- LML, gradient, alpha, mu / sigma, the full-form gradient, candidates bit-equal to single calls, Absorb + Produce -- for
    every kernel family, at the edge sizes 1 and 128, and the general sweep takes over at 129."""
    rng = np.random.default_rng(len(name))
    x = np.log(np.array(list(ts) + list(tn)))
    for n in (1, 20, 128, 129):
        X, y = _data(rng, n, D)
        Z = rng.uniform(-0.1, 1.1, (5, D))
        out = {}
        for tiny in (0, 1):
            g = gpmod.GP(D, simil, noise, X=X, Y=y)
            g.set_option("tiny", tiny)
            lml = g.Observe(x)
            grad = g.Gradient()
            alpha = g.Alpha.copy()
            mu, sg = g.Produce(Z)
            xs = np.stack([x, x + 0.02, x - 0.03])
            cl, cg, cs = g.observe_gradient_candidates(xs)
            assert list(cs) == [0, 0, 0] and cl[0] == lml
            np.testing.assert_array_equal(cg[0], grad)
            ThS, ThN = np.exp(x[:len(ts)]), np.exp(x[len(ts):])
            g.ThetaSimil, g.ThetaNoise = ThS, ThN
            g.Absorb(X, y)
            mu_a, sg_a = g.Produce(Z)
            full = np.concatenate([x, X.ravel(), y])
            lml_f = g.Observe(full)
            grad_f = g.Gradient()
            out[tiny] = (lml, grad, alpha, mu, sg, mu_a, sg_a, lml_f, grad_f, g.L.copy())
            g.close()
        a, b = out[0], out[1]
        # (default_noise: cond(K) ~ 1e10 -- two orders of summation differ by cond x eps there)
        tl, tv = (1e-7, 1e-4) if name == "default_noise" else (1e-12, 1e-8)
        assert abs(a[0] - b[0]) <= tl * max(1.0, abs(a[0])) and abs(a[7] - b[7]) <= tl * max(1.0, abs(a[7]))
        for k in (1, 2, 3, 4, 5, 6, 8, 9):
            np.testing.assert_allclose(b[k], a[k], rtol=tv, atol=tv * 0.1 * max(1.0, np.abs(a[k]).max()))
        if n == 129:   # above 128 both handles ran the general sweep
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[1], b[1])
    # not positive definite (gp/gp.go:228-230) through the one-launch form: the failing pivot as everywhere
    Xd = 100.0 * np.arange(40, dtype=float)[:, None] * np.ones((1, D))
    Xd[-1] = Xd[-2]
    g = gpmod.GP(D, kernel.Normal if D == 1 else kernel.Scaled(kernel.Normal), kernel.ConstantNoise(0.0),
                 ThetaSimil=[1.0] if D == 1 else [1.0, 1.0])
    with pytest.raises(gpmod.FactorizeError) as ei:
        g.Absorb(Xd, np.ones(40))
    assert ei.value.pivot == 39
    g.close()


def _same_results(a, b):
    assert abs(a[0] - b[0]) <= 1e-12 * max(1.0, abs(a[0]))
    np.testing.assert_allclose(b[1], a[1], rtol=1e-9, atol=1e-9 * np.abs(a[1]).max())
    np.testing.assert_allclose(b[2], a[2], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b[3], a[3], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(b[4], a[4], rtol=1e-9, atol=1e-9 * np.abs(a[4]).max())
    np.testing.assert_allclose(b[5], a[5], rtol=0, atol=1e-12 * np.abs(a[5]).max())
    np.testing.assert_allclose(b[6], a[6], rtol=1e-12)
    np.testing.assert_allclose(b[7], a[7], rtol=1e-9, atol=1e-9 * np.abs(a[7]).max())
    assert a[8] == b[8] == [0, 0, 0]
    np.testing.assert_allclose(b[9], a[9], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b[10], a[10], rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize("n,D", [(1, 1), (129, 1), (700, 2), (1500, 3), (4096, 4)])
def test_one_launch_chain_step_matches_the_256_block_kernel(gpmod, n, D):
    """Option chain_split (gp/gp.go:228-230, the diagonal-block work of Factorize): form 2, the chain per 128 columns in
    one launch (panel128.hip) with the 256 x 256 block inverses formed off the chain, against form 0, the one-workgroup
    256-block kernel: the same factor (rows of L), alpha, LML (1e-12 as VERDICT round 4 asks), gradient, mu / sigma;
    candidates; the failing pivot.  The removed form 1 and options chain_tail / inv_prio are refused."""
    rng = np.random.default_rng(n + D)
    X, y = _data(rng, n, D)
    Z = rng.uniform(-0.1, 1.1, (9, D))
    simil, noise = kernel.Scaled(kernel.Matern32), kernel.UniformNoise
    x = np.log([1.2, 0.5, 0.2])
    out = {}
    for split in (0, 2):
        g = gpmod.GP(D, simil, noise, X=X, Y=y)
        g.set_option("chain_split", split)
        lml = g.Observe(x)
        grad = g.Gradient()
        mu, sg = g.Produce(Z)
        xs = np.stack([x, x + 0.03, x - 0.02])
        cl, cg, cs = g.observe_gradient_candidates(xs)
        g.Absorb(X, y)                      # no gradient preparation: the lazy paths read the same block inverses
        mu_a, sg_a = g.Produce(Z)
        out[split] = (lml, grad, mu, sg, g.Alpha.copy(), g.L.copy(), cl, cg, list(cs), mu_a, sg_a)
        g.close()
    _same_results(out[0], out[2])
    # the failing pivot is reported from whichever half meets it (gp/gp.go:228-230): inputs so far apart that K = I in
    # floating point, the last one duplicated -- the last pivot is exactly 1 - 1 = 0 on every path
    for m in (2, 130, 200, 300):
        Xd = 100.0 * np.arange(m, dtype=float)[:, None]
        Xd[-1] = Xd[-2]
        for split in (0, 2):
            g = gpmod.GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0])
            g.set_option("chain_split", split)
            with pytest.raises(gpmod.FactorizeError) as ei:
                g.Absorb(Xd, np.ones(m))
            assert ei.value.pivot == m - 1
            g.close()
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    for name, value in (("chain_split", 1), ("chain_tail", 0), ("inv_prio", 0)):
        with pytest.raises(gpmod.GogpError):
            g.set_option(name, value)
    g.close()


def test_not_positive_definite(gpmod):
    """Duplicate inputs with zero noise: Factorize fails (gp/gp.go:228-230)."""
    X = np.array([[0.0], [0.0], [1.0]])
    y = np.array([1.0, 1.0, 0.0])
    g = gpmod.GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0])
    with pytest.raises(gpmod.FactorizeError) as ei:
        g.Absorb(X, y)
    assert ei.value.pivot == 1
    with pytest.raises(gpmod.FactorizeError):
        g.Observe(np.array([0.0]))


def test_no_observations(gpmod):
    """gp/gp.go:101-104,343-347,427-430."""
    g = gpmod.GP(2, kernel.Scaled(kernel.Normal), kernel.UniformNoise)
    g.X, g.Y = np.zeros((0, 2)), np.zeros(0)
    assert g.Observe(np.log([2.0, 1.0, 0.1])) == 0.0
    np.testing.assert_array_equal(g.Gradient(), np.zeros(3))
    mu, sigma = g.Produce([[0.1, 0.2], [0.5, 0.5]])
    np.testing.assert_array_equal(mu, np.zeros(2))
    np.testing.assert_allclose(sigma, np.sqrt([2.0, 2.0]), rtol=1e-15)


def test_observe_len_x(gpmod):
    g = gpmod.GP(2, kernel.Normal, kernel.ConstantNoise(0.1))
    with pytest.raises(ValueError):
        g.Observe(np.zeros(1 + 4))  # gp/gp.go:398-400


def test_repeated_observe_changes_theta(gpmod):
    """Every Observe re-runs the whole path (no stale caches across calls)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(2)
    D, n = 3, 400
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    for k in range(4):
        x = np.log([1.0 + 0.1 * k, 0.7 - 0.05 * k, 0.1 + 0.02 * k])
        lml, lml_o = g.Observe(x), o.Observe(x)
        assert abs(lml - lml_o) <= 1e-8 * abs(lml_o)
        if k % 2 == 0:
            go = o.Gradient()
            assert np.abs(g.Gradient() - go).max() <= 1e-6 * max(1, np.abs(go).max())


def test_barebones_csv_config1(gpmod, golden_dir):
    """BASELINE config 1: tutorial/data/barebones.csv, c*Matern32 + 0.01*UniformNoise."""
    from oracle.oracle import Oracle
    data = np.loadtxt(os.path.join(golden_dir, "barebones.csv"), delimiter=",")
    X, y = data[:, :1], data[:, 1]
    y = (y - y.mean()) / y.std()
    simil, noise = kernel.Scaled(kernel.Matern32), kernel.ScaledNoise(0.01)
    g = gpmod.GP(1, simil, noise, X=X, Y=y)
    o = Oracle(1, simil, noise)
    o.set_data(X, y)
    x = np.zeros(3)
    assert abs(g.Observe(x) - o.Observe(x)) < 1e-9
    np.testing.assert_allclose(g.Gradient(), o.Gradient(), rtol=1e-8, atol=1e-9)


def _factor_check(g, y, krow_fn, lml, rng, nrows=6):
    """Checks usable at sizes the oracle cannot reach: (a) sampled rows of L reproduce the Gram
    matrix, sum_k L_ik L_jk = K_ij for every j <= i of the sampled rows i (K rows rebuilt on
    the host from the kernel formula, noise on the diagonal), with the rows of L for the
    sampled columns fetched as well; (b) the log-determinant 2 sum_i log L_ii recomputed on
    the host from the downloaded diagonal, together with y^T alpha, reproduces the LML value
    the library returned (gp/gp.go:244-253)."""
    n = len(y)
    rows = np.unique(np.concatenate([rng.integers(0, n, nrows), [0, n - 1]]))
    Lr = g.L_rows(rows)  # len(rows) x n
    for a, i in enumerate(rows):
        krow = krow_fn(i)
        # (L L^T)_ij for the sampled j: needs row j of L as well -> use pairs inside `rows`
        for b, j in enumerate(rows):
            if j > i:
                continue
            got = float(Lr[a, : j + 1] @ Lr[b, : j + 1])
            assert abs(got - krow[j]) <= 1e-10 * max(1.0, abs(krow[j])), (i, j, got, krow[j])
        # ... and the row norm: (L L^T)_ii = K_ii
        assert abs(float(Lr[a] @ Lr[a]) - krow[i]) <= 1e-10 * krow[i]
    d = g.L_diag()
    assert np.all(d > 0)
    logdet = 2.0 * float(np.log(d).sum())
    lml_host = -0.5 * n * math.log(2 * math.pi) - 0.5 * logdet - 0.5 * float(y @ g.Alpha)
    assert abs(lml_host - lml) <= 1e-9 * abs(lml), (lml_host, lml)


def test_config3_full_size_properties(gpmod):
    """BASELINE config 3 (N=16384, D=8, RBF + white noise, fp64) at FULL size through
    size-independent properties (the oracle does not finish in seconds at this N):
      1. K alpha = y on sampled rows (K rows rebuilt on the host from the kernel formula);
      2. the gradient agrees with a central difference of LML along a random direction;
      3. Produce at the training inputs: mu_i = y_i - s2 alpha_i exactly (K alpha = y), and
         sum_i sigma_i^2 = N s2 - s2^2 tr(K^-1), with tr(K^-1) taken from the noise component
         of the gradient (dLML/dlog s = s2 (alpha.alpha - tr K^-1)) -- a checksum tying
         Absorb/Observe, Gradient and Produce together."""
    from gogp_amd import synth
    N, D = 16384, 8
    X, y = synth.make_inputs(N, D, 20251116)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    th = synth.theta0(D)
    x = np.log(th)
    lml = g.Observe(x)
    grad = g.Gradient()
    alpha = g.Alpha
    c, l, s = th
    s2 = s * s
    # 1. K alpha = y on sampled rows
    rng = np.random.default_rng(1)
    for i in rng.integers(0, N, 24):
        r2 = ((X[i] - X) ** 2).sum(1) / (l * l)
        krow = c * np.exp(-0.5 * r2)
        krow[i] += s2
        assert abs(krow @ alpha - y[i]) <= 1e-8 * max(1.0, np.abs(krow * alpha).sum()), i
    # 1b. the factor itself and the log-determinant behind the LML value

    def krow3(i):
        kr = c * np.exp(-0.5 * ((X[i] - X) ** 2).sum(1) / (l * l))
        kr[i] += s2
        return kr
    _factor_check(g, y, krow3, lml, rng)
    # 2. directional derivative
    v = rng.normal(size=3)
    v /= np.linalg.norm(v)
    h = 1e-4
    fd = (g.Observe(x + h * v) - g.Observe(x - h * v)) / (2 * h)
    assert abs(fd - grad @ v) <= 1e-6 * max(1.0, abs(fd)), (fd, grad @ v)
    # 3. Produce at the training inputs
    g.Observe(x)
    mu, sigma = g.Produce(X)
    np.testing.assert_allclose(mu, y - s2 * alpha, rtol=0, atol=1e-8 * max(1.0, np.abs(y).max()))
    tr_kinv = float(alpha @ alpha) - grad[2] / s2
    want = N * s2 - s2 * s2 * tr_kinv
    got = float((sigma ** 2).sum())
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert np.isfinite(lml)


@pytest.mark.parametrize("shape", ["config4", "config5"])
def test_config4_config5_shapes_full_size_properties(gpmod, shape):
    """The shapes of BASELINE configs 4 (Matern-5/2, reference coefficient, N=32768, D=16) and
    5 (ARD-RBF, N=65536, D=32, P=34; here in fp64 -- as configured, in fp32, it runs in
    test_config5_as_configured_fp32_full_size below) on ONE GPU, through
    the same size-independent properties as config 3: K alpha = y on sampled rows rebuilt on
    the host, gradient against a central difference of the LML along a random direction,
    and Produce at training inputs (mu_i = y_i - s2 alpha_i)."""
    from gogp_amd import synth
    if shape == "config4":
        N, D = 32768, 16
        simil = kernel.Scaled(kernel.Matern52)
        th = np.array([1.0, math.sqrt(D / 6.0), 0.1])

        def krow_fn(i, X):
            r = np.sqrt(((X[i] - X) ** 2).sum(1)) / th[1]
            return th[0] * (1 + math.sqrt(5) * r + r * r) * np.exp(-math.sqrt(5) * r)  # kernel.go:89-92
    else:
        N, D = 65536, 32
        simil = kernel.Scaled(kernel.ARD(kernel.Normal, D))
        ls = math.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D))
        th = np.concatenate([[1.0], ls, [0.1]])

        def krow_fn(i, X):
            return th[0] * np.exp(-0.5 * (((X[i] - X) / ls) ** 2).sum(1))
    X, y = synth.make_inputs(N, D, 20251114 + (3 if shape == "config4" else 4))
    g = gpmod.GP(D, simil, kernel.UniformNoise, X=X, Y=y)
    x = np.log(th)
    s2 = th[-1] ** 2
    lml = g.Observe(x)
    grad = g.Gradient()
    assert np.isfinite(lml) and grad.shape == x.shape
    alpha = g.Alpha
    rng = np.random.default_rng(2)
    for i in rng.integers(0, N, 8):
        krow = krow_fn(i, X)
        krow[i] += s2
        assert abs(krow @ alpha - y[i]) <= 1e-8 * max(1.0, np.abs(krow * alpha).sum()), i

    def krow_noise(i):
        kr = krow_fn(i, X)
        kr[i] += s2
        return kr
    _factor_check(g, y, krow_noise, lml, rng, nrows=4)
    v = rng.normal(size=len(x))
    v /= np.linalg.norm(v)
    h = 1e-4
    fd = (g.Observe(x + h * v) - g.Observe(x - h * v)) / (2 * h)
    assert abs(fd - grad @ v) <= 1e-6 * max(1.0, abs(fd)), (fd, grad @ v)
    g.Observe(x)
    idx = rng.integers(0, N, 1024)
    mu, sigma = g.Produce(X[idx])
    np.testing.assert_allclose(mu, (y - s2 * alpha)[idx], rtol=0, atol=1e-8 * max(1.0, np.abs(y).max()))
    assert np.all(np.isfinite(sigma)) and np.all(sigma < th[-1] * 1.0001)  # latent sd at a training input < noise sd
    g.close()


def test_config5_as_configured_fp32_full_size(gpmod):
    """BASELINE configs[4] AS CONFIGURED: ARD-RBF, N = 65536, D = 32, precision = 32 (float matrices and
    fp32 MFMA products, fp64 inputs / diagonal blocks / reductions / refinement of alpha; DESIGN.md
    section 6), on one GPU.  Size-independent properties of the fp32 result itself -- K alpha = y on
    sampled rows rebuilt on the host, the LML from the downloaded diagonal of the factor and y^T alpha,
    Produce at training inputs -- and the fp64 path on the same data as the yardstick for LML, gradient
    and alpha, within the bounds DESIGN.md section 6 states for this size."""
    from gogp_amd import synth
    N, D = 65536, 32
    simil = kernel.Scaled(kernel.ARD(kernel.Normal, D))
    ls = math.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D))
    th = np.concatenate([[1.0], ls, [0.1]])
    x = np.log(th)
    s2 = th[-1] ** 2
    X, y = synth.make_inputs(N, D, 20251114 + 4)
    g32 = gpmod.GP(D, simil, kernel.UniformNoise, X=X, Y=y, precision=32)
    lml32 = g32.Observe(x)
    grad32 = g32.Gradient()
    a32 = g32.Alpha
    assert np.isfinite(lml32) and np.isfinite(grad32).all() and grad32.shape == x.shape
    rng = np.random.default_rng(5)
    # K alpha = y with the exact (fp64, host) rows of K: alpha was refined against the exact Gram matrix
    for i in rng.integers(0, N, 8):
        krow = th[0] * np.exp(-0.5 * (((X[i] - X) / ls) ** 2).sum(1))
        krow[i] += s2
        assert abs(krow @ a32 - y[i]) <= 2e-5 * max(1.0, np.abs(krow * a32).sum()), i
    # the LML from its parts: log-determinant from the downloaded (float) diagonal, quadratic term y^T alpha
    d = g32.L_diag()
    assert d.shape == (N,) and np.all(d > 0)
    lml_parts = -0.5 * N * math.log(2 * math.pi) - np.log(d).sum() - 0.5 * float(y @ a32)
    assert abs(lml_parts - lml32) <= 2e-6 * abs(lml32), (lml_parts, lml32)
    idx = rng.integers(0, N, 512)
    mu, sigma = g32.Produce(X[idx])
    np.testing.assert_allclose(mu, (y - s2 * a32)[idx], rtol=0, atol=2e-3 * max(1.0, np.abs(y).max()))
    assert np.all(np.isfinite(sigma)) and np.all(sigma < th[-1] * 1.01)
    # the fp64 path on the same data (96 GB next to the 48 GB of the fp32 handle: both fit one MI355X)
    g64 = gpmod.GP(D, simil, kernel.UniformNoise, X=X, Y=y)
    lml64 = g64.Observe(x)
    grad64 = g64.Gradient()
    a64 = g64.Alpha
    assert abs(lml32 - lml64) <= 2e-6 * abs(lml64), (lml32, lml64)                      # measured 7.5e-7
    assert np.abs(grad32 - grad64).max() <= 5e-4 * np.abs(grad64).max(), (grad32, grad64)  # measured 1.2e-4
    assert np.abs(a32 - a64).max() <= 1e-4 * np.abs(a64).max()                          # measured 2.2e-5
    g32.close()
    g64.close()


@pytest.mark.parametrize("opts", [
    {"lookahead": 0}, {"eager": 0}, {"superpanel": 1}, {"superpanel": 3}, {"superpanel": 4}, {"superpanel": 8},
    {"superpanel": 6, "eager": 0},
    {"lookahead": 0, "superpanel": 4},
    {"kinv_fused": 0}, {"kinv_fused": 1}, {"kinv_fused": 1, "superpanel": 3}, {"ktri": 0},
    {"superpanel_head": 3, "head_remaining": 2}, {"superpanel_head": 4, "head_remaining": 0},
    {"superpanel_head": 3, "head_remaining": 4, "kinv_fused": 1}, {"superpanel_head": 5, "head_remaining": 3, "eager": 0},
], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("n", [300, 2300])
def test_schedule_options_same_results(gpmod, opts, n):
    """Every scheduling option (stream layout, super-panel width, lazy inverse) computes the same numbers as the default schedule; only the grouping of the
    rank-k updates -- hence rounding -- may differ."""
    rng = np.random.default_rng(n)
    D = 3
    X, y = _data(rng, n, D)
    Z = rng.uniform(0, 1, (11, D))
    x = np.log([1.1, 0.5, 0.2])
    ref = gpmod.GP(D, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, X=X, Y=y)
    lml0, g0 = ref.Observe(x), ref.Gradient()
    mu0, sg0 = ref.Produce(Z)
    g = gpmod.GP(D, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, X=X, Y=y)
    for k, v in opts.items():
        g.set_option(k, v)
    for _ in range(2):  # twice: state carried from one evaluation into the next
        lml, grad = g.Observe(x), g.Gradient()
        mu, sg = g.Produce(Z)
        assert abs(lml - lml0) <= 1e-10 * max(1.0, abs(lml0))
        np.testing.assert_allclose(grad, g0, rtol=1e-8, atol=1e-8 * np.abs(g0).max())
        np.testing.assert_allclose(mu, mu0, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(sg, sg0, rtol=1e-8, atol=1e-11)
    g.close()
    ref.close()


def test_anynoise_constant_noise_with_parameter(gpmod):
    """tutorial/anynoise/kernel/kernel.go:26-35: constant 1e-5 noise variance that still owns one
    parameter (NTheta() == 1) which K does not depend on: its gradient component is exactly 0
    and the LML does not move with it; hyperparameters-only and full (withObs) forms."""
    from cases import ANYNOISE
    from oracle.oracle import Oracle
    name, D, simil, noise, ts, tn = ANYNOISE
    g, o = _check_against(gpmod, Oracle, name, D, simil, noise, ts, tn, n=40, m=7, seed=11)
    x = np.log(np.array(ts + tn))
    lml = g.Observe(x)
    grad = g.Gradient()
    o.Observe(x)  # the oracle's Gradient consumes dK like the reference's (gp/gp.go:496)
    assert grad[2] == 0.0 and o.Gradient()[2] == 0.0
    x2 = x.copy()
    x2[2] += 1.7
    assert g.Observe(x2) == lml
    # full form, as the anynoise case study drives it (tutorial/tutorial.go:101-108)
    rng = np.random.default_rng(3)
    X, y = _data(rng, 12, D)
    xf = np.concatenate([x, X.reshape(-1), y])
    gf = gpmod.GP(D, simil, noise)
    of = Oracle(D, simil, noise)
    assert abs(gf.Observe(xf) - of.Observe(xf)) <= 1e-9 * max(1.0, abs(of.Observe(xf)))
    np.testing.assert_allclose(gf.Gradient(), of.Gradient(), rtol=1e-6, atol=1e-7)


def test_config1_barebones_recipe_64_rows(gpmod):
    """BASELINE configs[0] as worded: 1-D Normal kernel, N = 64 rows made by the recipe of the
    reference's tutorial/data/barebones.csv (x = i*pi/10, y = sin x + noise); HIP path vs the
    faithful oracle (the 20-row file itself with the tutorial's c*Matern32 kernel is
    test_barebones_csv_config1)."""
    from gogp_amd import configs
    from oracle.oracle import Oracle
    wl = configs.workload(1)
    X, y = wl.inputs()
    assert X.shape == (64, 1)
    g = gpmod.GP(1, wl.simil, wl.noise, X=X, Y=y)
    o = Oracle(1, wl.simil, wl.noise)
    o.set_data(X, y)
    for k in range(3):
        x = wl.log_theta(k)
        lml, lml_o = g.Observe(x), o.Observe(x)
        assert abs(lml - lml_o) <= 1e-9 * max(1.0, abs(lml_o))
        np.testing.assert_allclose(g.Gradient(), o.Gradient(), rtol=1e-7, atol=1e-8)
    Z = wl.test_points(16)
    mu, sg = g.Produce(Z)
    mu_o, sg_o = o.Produce(Z)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(sg, sg_o, rtol=1e-6, atol=1e-8)


def test_condition_error_like_gonum(gpmod):
    """gonum's Cholesky solves return a Condition error above mat.ConditionTolerance (1e16),
    which gp/gp.go:233-236 passes on; here (max L_ii / min L_ii)^2 is compared with the limit.
    With the limit lowered an ordinary matrix trips it deterministically: the error is raised
    AFTER the state was stored (as gonum fills the result and returns the error)."""
    rng = np.random.default_rng(59)
    n, D = 300, 2
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    x = np.log([1.0, 0.6, 0.05])
    ref = gpmod.GP(D, simil, noise, X=X, Y=y)
    lml_ref, alpha_ref = ref.Observe(x), ref.Alpha
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    assert g.Observe(x) == lml_ref  # default limit 1e16: fine
    g.set_option("cond_limit_log10", 1)
    with pytest.raises(gpmod.ConditionError):
        g.Observe(x)
    assert g.LML() == lml_ref
    np.testing.assert_array_equal(g.Alpha, alpha_ref)
    np.testing.assert_array_equal(g.Gradient(), ref.Gradient())
    g.ThetaSimil, g.ThetaNoise = list(np.exp(x[:2])), list(np.exp(x[2:]))
    with pytest.raises(gpmod.ConditionError):
        g.Absorb(X, y)
    g.set_option("cond_limit_log10", 16)
    g.Absorb(X, y)
    assert g.LML() == lml_ref


@pytest.mark.parametrize("shape", ["config5", "config3"])
def test_fp32_path_accuracy_contract(gpmod, shape):
    """BASELINE configs[4] is an fp32 configuration.  The fp32 path (option precision = 32) keeps
    the N x N matrices and the O(N^3) products in fp32 (v_mfma_f32_32x32x2_f32) and everything
    else -- inputs, kernel evaluation, 256x256 diagonal blocks, log-determinant, substitutions,
    one step of iterative refinement of alpha against the exact Gram matrix, gradient sums --
    in fp64.  Contract against the fp64 oracle (DESIGN.md "fp32 path"; measured values are
    5-20x below these bounds):
        config-5 shape (ARD-RBF, D=32):  LML 2e-6 rel, gradient 2e-5 of max|g|, alpha 2e-5,
                                         mu 1e-3, sigma 1e-4
        config-3 shape (RBF, D=8, cond(K) 10x larger): LML 1e-5, gradient 1e-4"""
    from gogp_amd import configs
    from oracle.oracle import FastOracle
    n = 4096
    wl = configs.workload(5 if shape == "config5" else 3, n)
    X, y = wl.inputs()
    Z = wl.test_points(64)
    x = wl.log_theta(0)
    o = FastOracle(wl.D, wl.simil, wl.noise)
    o.set_data(X, y)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    mu_o, sg_o = o.Produce(Z)
    g = gpmod.GP(wl.D, wl.simil, wl.noise, X=X, Y=y, precision=32)
    lml, grad = g.Observe(x), g.Gradient()
    mu, sg = g.Produce(Z)
    tol_lml, tol_grad = (2e-6, 2e-5) if shape == "config5" else (1e-5, 1e-4)
    assert abs(lml - lml_o) <= tol_lml * abs(lml_o), (lml, lml_o)
    assert np.abs(grad - grad_o).max() <= tol_grad * np.abs(grad_o).max(), (grad, grad_o)
    assert np.abs(g.Alpha - o.Alpha).max() <= 2e-5 * np.abs(o.Alpha).max()
    assert np.abs(mu - mu_o).max() <= 1e-3 * np.abs(mu_o).max()
    assert np.abs(sg - sg_o).max() <= 2e-4 * np.abs(sg_o).max()
    # the factor is exported in fp64 whatever the storage type: L L^T = K to fp32 accuracy
    rows = np.array([0, 17, n - 1])
    Lr = g.L_rows(rows)
    th = np.exp(x)
    for a, i in enumerate(rows):
        kii = th[0] + th[-1] ** 2
        assert abs(float(Lr[a] @ Lr[a]) - kii) <= 1e-5 * kii
    d = g.L_diag()
    assert d.shape == (n,) and np.all(d > 0)
    # second evaluation on the same handle, then Absorb (lazy path) agree with the first
    assert abs(g.Observe(x) - lml) <= 1e-12 * abs(lml)
    g.ThetaSimil, g.ThetaNoise = list(th[:-1]), [float(th[-1])]
    g.Absorb(X, y)
    assert abs(g.LML() - lml) <= 1e-9 * abs(lml)
    # what the fp32 path does not offer fails loudly
    xf = np.concatenate([x, X[:8].reshape(-1), y[:8]])
    g8 = gpmod.GP(wl.D, wl.simil, wl.noise, precision=32)
    g8.Observe(xf)
    with pytest.raises(gpmod.GogpError):
        g8.Gradient()  # full Observe form: fp64 only
    g.close()
    g8.close()


@pytest.mark.parametrize("m", [1, 7, 16, 40])
def test_fp32_produce_for_few_test_points(gpmod, m):
    """gp/gp.go:322-357 on the fp32 path with M <= 16 test points (above: the float tile-kernel chain, which the last case
    checks against itself): the one-pass persistent substitution (trsm_small.hip)
    reads the FLOAT factor and block inverses, widens them in registers and sums in fp64 -- inside the fp32 contract
    against the oracle (mu 1e-3, sigma 2e-4 of their largest values) and no worse than the float tile-kernel chain it
    replaces (option produce_small_max = 0)."""
    from gogp_amd import configs
    from oracle.oracle import FastOracle
    n = 2500
    wl = configs.workload(5, n)
    X, y = wl.inputs()
    Z = wl.test_points(m)
    x = wl.log_theta(0)
    o = FastOracle(wl.D, wl.simil, wl.noise)
    o.set_data(X, y)
    o.Observe(x)
    mu_o, sg_o = o.Produce(Z)
    g = gpmod.GP(wl.D, wl.simil, wl.noise, X=X, Y=y, precision=32)
    g.Observe(x)
    mu, sg = g.Produce(Z)
    g.set_option("produce_small_max", 0)
    mu_c, sg_c = g.Produce(Z)
    g.close()
    e_mu, e_sg = np.abs(mu - mu_o).max() / np.abs(mu_o).max(), np.abs(sg - sg_o).max() / np.abs(sg_o).max()
    c_mu, c_sg = np.abs(mu_c - mu_o).max() / np.abs(mu_o).max(), np.abs(sg_c - sg_o).max() / np.abs(sg_o).max()
    assert e_mu <= 1e-3 and e_sg <= 2e-4, (e_mu, e_sg)
    assert e_mu <= 2.0 * c_mu + 1e-6 and e_sg <= 2.0 * c_sg + 1e-6, (e_mu, c_mu, e_sg, c_sg)


def test_fp32_gradient_ill_conditioned_case(gpmod, golden_dir):
    """The case round 3's randomised stress run found (tools/stress.py 360 7: Matern-3/2, N = 1721, D = 2, data kept
    in tests/golden/fp32_illcond_matern32.npz with the oracle's gradient and what the fp32 path returned then): LML
    2e-6, but the gradient off by 3.6e-3 of its largest component -- all of it in the OUTPUT-SCALE component (-0.7836
    against -0.8503; length scale 7e-6, noise 2.4e-4), which the reduction forms as a sum over W = alpha alpha^T -
    K^-1 that cancels to a few 1e-3 of its terms.  Round 3 widened the stress tolerance; round 4 takes that component
    from its closed form tr(W (K - v I)) = y^T alpha - n - v tr(W) and tr(W) from fp64 sums over Y = L^-T (api.hip:
    fp32_gradient_identities).  What was left then, the noise component's 1.5e-4 -- tr(K^-1) of a float factor whose
    DIAGONAL is biased (tools/fp32_bias_probe.py) -- went in round 5 with the diagonal blocks' trailing updates summed in
    fp64 (diagsyrk.hip, option diag_fp64): every component inside the 1e-4 the reference checks its own gradient to
    (gp_test.go:170,248)."""
    from oracle.oracle import FastOracle
    d = np.load(os.path.join(golden_dir, "fp32_illcond_matern32.npz"))
    X, y, x = d["X"], d["y"], d["x"]
    simil, noise = [c for c in CASES if c[0] == "matern32"][0][2:4]
    o = FastOracle(2, simil, noise)
    o.set_data(X, y)
    lml_o, grad_o = o.Observe(x), o.Gradient()
    np.testing.assert_allclose(grad_o, d["grad_oracle"], rtol=1e-9)
    scale = np.abs(grad_o).max()
    assert np.abs(d["grad_fp32_round3"] - grad_o).max() / scale > 3e-3  # what it was
    for opts in ({}, {"eager": 0}):
        g = gpmod.GP(2, simil, noise, X=X, Y=y, precision=32)
        for k, v in opts.items():
            g.set_option(k, v)
        lml = g.Observe(x)
        grad = g.Gradient()
        assert abs(lml - lml_o) <= 1e-5 * abs(lml_o)
        err = np.abs(grad - grad_o) / scale
        assert err[0] <= 1e-4 and err[1] <= 1e-4 and err[2] <= 1e-4, (grad, grad_o, err)  # measured 3.3e-5, 2.7e-6, 6.5e-5
        g.set_option("trace_fp64", 0)  # round 3's sums, on the same factor
        g.Observe(x)
        assert np.abs(g.Gradient() - grad_o).max() / scale > 1e-3
        g.set_option("trace_fp64", 1)
        g.set_option("diag_fp64", 0)   # round 4's pivots: the float matrix's own diagonal blocks
        g.Observe(x)
        assert 1e-4 < np.abs(g.Gradient() - grad_o).max() / scale < 5e-4
        g.close()


@pytest.mark.parametrize("n,D,eager", [(1500, 3, 1), (4096, 4, 1), (2300, 2, 0)])
def test_mixed_precision_gradient_option(gpmod, n, D, eager):
    """Option gradient_precision = 32 on an fp64 handle: the factorisation and the LML are the fp64 path's bit for bit,
    alpha and Produce fp64 as well; only Y = L^-T and K^-1 = Y Y^T -- what the gradient alone needs, 2/3 of the flops -- run on the fp32
    tile kernel from a float copy of the fp64 factor, and the trace / scale components come from their closed forms
    (api.hip: mixed gradient, fp32_gradient_identities).  The reference checks its own gradient to 1e-4
    (gp_test.go:170,248); here it stays within 1e-6 of the oracle's.  Never the default, never bench.py's `value`."""
    # a SUM of terms has no closed form for its scale components: the option is refused there (round 5; round 4 shipped
    # 1.9e-4 under a 1e-3 bound), and so it is for a kernel without an output scale
    for sm, nz in ((kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.Normal)]), kernel.UniformNoise),
                   (kernel.Normal, kernel.ConstantNoise(0.1))):
        gs = gpmod.GP(1, sm, nz)
        with pytest.raises(gpmod.GogpError):
            gs.set_option("gradient_precision", 32)
        gs.set_option("gradient_precision", 64)
        gs.close()
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(n + D)
    X, y = _data(rng, n, D)
    Z = rng.uniform(0, 1, (40, D))
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    x = np.log([1.0, math.sqrt(D / 6.0), 0.1])
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    g.set_option("eager", eager)
    lml64, grad64, alpha64 = g.Observe(x), g.Gradient(), g.Alpha
    mu64, sigma64 = g.Produce(Z)
    g.set_option("gradient_precision", 32)
    lml, grad = g.Observe(x), g.Gradient()
    assert lml == lml64
    # alpha: by backward substitution with the fp64 factor (the native fused sweep takes alpha = Y z from the fp64 Y
    # it no longer has) -- the same vector to rounding, and with it Produce
    np.testing.assert_allclose(g.Alpha, alpha64, rtol=1e-10, atol=1e-12 * np.abs(alpha64).max())
    mu, sigma = g.Produce(Z)
    np.testing.assert_allclose(mu, mu64, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(sigma, sigma64, rtol=1e-9, atol=1e-11)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    o.Observe(x)
    grad_o = o.Gradient()
    scale = np.abs(grad_o).max()
    assert np.abs(grad - grad_o).max() <= 1e-6 * scale, (grad, grad_o)
    assert np.abs(grad64 - grad_o).max() <= 1e-8 * scale
    np.testing.assert_array_equal(g.Gradient(), grad)  # cached, repeatable
    g.set_option("gradient_precision", 64)             # and back: the fp64 inverse again
    assert g.Observe(x) == lml64
    np.testing.assert_array_equal(g.Gradient(), grad64)
    g.close()


def test_observe_gradient_batch_matches_single_calls(gpmod):
    """k candidates evaluated at once (one host thread per handle) give bit for bit what the
    same handles return one at a time."""
    rng = np.random.default_rng(53)
    n, D, k = 1200, 3, 4
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Matern32), kernel.UniformNoise
    xs = np.log(np.array([[1.0, 0.5, 0.2], [1.2, 0.6, 0.25], [0.8, 0.4, 0.15], [1.1, 0.7, 0.3]]))
    gps = [gpmod.GP(D, simil, noise, X=X, Y=y) for _ in range(k)]
    want = [(g.Observe(x), g.Gradient()) for g, x in zip(gps, xs)]
    for _ in range(3):
        lmls, grads = gpmod.observe_gradient_batch(gps, xs)
        for i in range(k):
            assert lmls[i] == want[i][0]
            np.testing.assert_array_equal(grads[i], want[i][1])
    np.testing.assert_array_equal(gps[2].Gradient(), want[2][1])  # the handles stay usable
    for g in gps:
        g.close()


@pytest.mark.parametrize("n,D,name", [(1200, 3, "matern32"), (700, 2, "periodic_sum"), (2100, 24, "ard"), (37, 1, "rbf"),
                                      (600, 24, "ard")])  # ARD below N = 1024: the MFMA reduction inside the captured graph
def test_candidates_in_one_launch_sequence_match_single_calls(gpmod, n, D, name):
    """gogp_observe_gradient_candidates: k parameter vectors in one launch sequence (candidate
    index on the grid's z axis) give bit for bit what Observe + Gradient return one at a time --
    the same kernels on the same data, only batched -- and leave the handle's own state alone."""
    rng = np.random.default_rng(77 + n)
    X, y = _data(rng, n, D)
    noise = kernel.UniformNoise
    simil = {"matern32": lambda: kernel.Scaled(kernel.Matern32), "rbf": lambda: kernel.Scaled(kernel.Normal),
             "periodic_sum": lambda: kernel.Sum([kernel.Scaled(kernel.Normal), kernel.Scaled(kernel.Periodic)]),
             "ard": lambda: kernel.Scaled(kernel.ARD(kernel.Normal, D))}[name]()
    P = simil.NTheta() + 1
    base = np.log(np.linspace(0.7, 1.3, P))
    base[-1] = np.log(0.2)
    k = 5
    xs = base[None, :] + 0.15 * rng.normal(size=(k, P))
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    want = [(g.Observe(x), g.Gradient()) for x in xs]
    lml_own, grad_own = g.Observe(base), g.Gradient()       # the handle's own state before the batch
    Z = rng.uniform(0, 1, (7, D))
    mu_own, sigma_own = g.Produce(Z)
    for rep in range(2):
        lmls, grads, status = g.observe_gradient_candidates(xs)
        assert list(status) == [0] * k
        for c in range(k):
            assert lmls[c] == want[c][0], (c, lmls[c], want[c][0])
            np.testing.assert_array_equal(grads[c], want[c][1])
    # untouched: LML, cached gradient, Produce of the handle's own factorisation
    assert g.LML() == lml_own
    np.testing.assert_array_equal(g.Gradient(), grad_own)
    mu2, sigma2 = g.Produce(Z)
    np.testing.assert_array_equal(mu2, mu_own)
    np.testing.assert_array_equal(sigma2, sigma_own)
    # the same call again and again with other parameters and, in between, other data of the same
    # size: up to N = 1024 the launch sequence becomes a hipGraph (built node by node, graphrec.h) on its second
    # use and is replayed from then on -- parameters and data must still be the current ones
    for rep in range(4):
        xs2 = base[None, :] + 0.1 * rng.normal(size=(k, P))
        if rep == 2:
            g.Y = y[::-1].copy()
        lmls, grads, status = g.observe_gradient_candidates(xs2)
        for c in (0, k - 1):
            assert lmls[c] == g.Observe(xs2[c])
            np.testing.assert_array_equal(grads[c], g.Gradient())
    g.Y = y
    g.Observe(base)
    # a smaller batch after a larger one, and a single candidate
    lmls, grads, status = g.observe_gradient_candidates(xs[1:3])
    assert lmls[0] == want[1][0] and lmls[1] == want[2][0]
    lmls, grads, status = g.observe_gradient_candidates(xs[4])
    assert lmls[0] == want[4][0]
    np.testing.assert_array_equal(grads[0], want[4][1])
    g.close()


@pytest.mark.parametrize("n,k", [(1500, 1), (4096, 1), (4096, 3), (8192, 1)])
def test_candidates_explicit_graph_with_the_sweeps_dependencies_is_bit_identical(gpmod, n, k):
    """Option graph = 2: the candidates' launch sequence as an EXPLICITLY built hipGraph -- hipGraphAddKernelNode /
    AddMemcpyNode / AddMemsetNode with the sweep's cross-stream dependencies as edges, no stream capture (graphrec.h) --
    at the sizes where the evaluation forks over six streams (round 2's stream capture died in hipStreamEndCapture
    there).  Same kernels, same arguments, a dependency set that contains the stream path's: every bit of LML and
    gradient equals the stream path's (graph = 0) and the single calls', over parameter changes between replays.
    (Not the default: this runtime runs parallel branches of a graph no faster than their serialisation, DESIGN.md.)"""
    rng = np.random.default_rng(n + k)
    D = 3
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    base = np.log([1.0, 0.7, 0.2])
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    xs_of = lambda r: base[None, :] + 0.02 * ((np.arange(k)[:, None] + r) % 5)
    g.set_option("graph", 0)
    want = [g.observe_gradient_candidates(xs_of(r)) for r in range(4)]
    assert g.graph_info() == (0, False)
    g.set_option("graph", 2)
    for r in range(4):  # built on the second identical use, replayed from then on
        lmls, grads, st = g.observe_gradient_candidates(xs_of(r))
        assert list(st) == [0] * k
        np.testing.assert_array_equal(lmls, want[r][0])
        np.testing.assert_array_equal(grads, want[r][1])
    nodes, refused = g.graph_info()
    assert not refused and nodes > 40, (nodes, refused)
    lml1 = g.Observe(xs_of(3)[0])  # and the single calls
    assert lml1 == want[3][0][0]
    np.testing.assert_array_equal(g.Gradient(), want[3][1][0])
    g.close()


@pytest.mark.parametrize("n,k", [(700, 3), (1500, 1), (1500, 3)])
def test_candidates_explicit_chain_in_enqueue_order_is_bit_identical(gpmod, n, k):
    """VERDICT round 4, item 4.  Round 4 tried an explicitly built LINEAR graph (every node behind the node added before
    it: the stream path's enqueue order, a linear extension of the DAG of option graph = 2) and saw gradients that were
    wrong and varied from run to run, unexplained.  Option graph = 3 is that chain built by the same recorder
    (graphrec.h): bit-identical to the streams here, over parameter changes between replays.  The symptom reproduces
    exactly -- in the chain AND in the DAG -- as soon as ONE operation of the launch sequence reaches the runtime
    directly instead of the recorder (tried with the copy of y into the substitution's work vector: executed once, at
    build time, and never at replay, so every replay substitutes into what the previous one left: DESIGN.md section 4);
    every copy / fill of the candidates' sequence goes through rec_memcpy_async / rec_memset_async."""
    rng = np.random.default_rng(n + k)
    D = 3
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    base = np.log([1.0, 0.7, 0.2])
    g = gpmod.GP(D, simil, noise, X=X, Y=y)
    xs_of = lambda r: base[None, :] + 0.02 * ((np.arange(k)[:, None] + r) % 5)
    g.set_option("graph", 0)
    want = [g.observe_gradient_candidates(xs_of(r)) for r in range(5)]
    g.set_option("graph", 3)
    for r in range(5):
        lmls, grads, st = g.observe_gradient_candidates(xs_of(r))
        assert list(st) == [0] * k
        np.testing.assert_array_equal(lmls, want[r][0])
        np.testing.assert_array_equal(grads, want[r][1])
    nodes, refused = g.graph_info()
    assert not refused and nodes > 40, (nodes, refused)
    g.close()


def test_candidates_on_the_fp32_path(gpmod):
    """precision = 32: the candidates go through ONE arena slot one after the other (the float kernels carry no
    candidate index); every bit equals the single fp32 Observe + Gradient calls, the handle's own factorisation is
    left alone, and the line search with k trial points per call follows the k = 1 path."""
    from gogp_amd import optimize
    rng = np.random.default_rng(99)
    n, D = 2100, 4
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.ARD(kernel.Normal, D)), kernel.UniformNoise
    base = np.log(np.concatenate([[1.0], np.full(D, 0.8), [0.2]]))
    xs = np.stack([base + 0.04 * c for c in range(4)])
    g = gpmod.GP(D, simil, noise, X=X, Y=y, precision=32)
    want = [(g.Observe(x), g.Gradient()) for x in xs]
    lml_own, grad_own = g.Observe(base - 0.1), g.Gradient()
    Z = rng.uniform(0, 1, (9, D))
    mu_own, sigma_own = g.Produce(Z)
    for rep in range(2):
        lmls, grads, st = g.observe_gradient_candidates(xs)
        assert list(st) == [0] * 4
        for c in range(4):
            assert lmls[c] == want[c][0]
            np.testing.assert_array_equal(grads[c], want[c][1])
    assert g.LML() == lml_own
    np.testing.assert_array_equal(g.Gradient(), grad_own)
    mu2, sigma2 = g.Produce(Z)
    np.testing.assert_array_equal(mu2, mu_own)
    np.testing.assert_array_equal(sigma2, sigma_own)
    r1 = optimize.lbfgs(g, base, major_iterations=3, gradient_threshold=1e-12)
    r3 = optimize.lbfgs(g, base, major_iterations=3, gradient_threshold=1e-12, line_search_candidates=3)
    np.testing.assert_array_equal(r1.x, r3.x)
    assert r1.history == r3.history
    g.close()


def test_candidates_graph_survives_arena_reallocation(gpmod):
    """The captured launch sequence holds raw pointers into the candidates' arena at ONE slot stride.
    (k=4, n=1000) sizes the arena for npad 1024; with n=500 on the same handle (k=4, n=500) twice
    captures a graph with that stride; k=8 at n=500 reallocates the arena with the slots of npad 512 --
    possibly at the same address; (k=4, n=500) again must not replay the stale graph (it would write past
    the new arena).  Reference values come from a handle that never captures (option graph = 0)."""
    rng = np.random.default_rng(4242)
    D = 2
    Xb, yb = _data(rng, 1000, D)
    Xs, ys = Xb[:500].copy(), yb[:500].copy()
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    xs8 = np.log([1.0, 0.5, 0.2])[None, :] + 0.1 * rng.normal(size=(8, 3))
    ref = gpmod.GP(D, simil, noise, X=Xs, Y=ys)
    ref.set_option("graph", 0)
    want = [(ref.Observe(x), ref.Gradient()) for x in xs8]
    ref.close()
    g = gpmod.GP(D, simil, noise, X=Xb, Y=yb)
    g.observe_gradient_candidates(xs8[:4])            # arena: 4 slots of npad 1024
    g.X, g.Y = Xs, ys

    def check(k):
        lmls, grads, status = g.observe_gradient_candidates(xs8[:k])
        assert list(status) == [0] * k
        for c in range(k):
            assert lmls[c] == want[c][0], (k, c)
            np.testing.assert_array_equal(grads[c], want[c][1])

    check(4)   # seen once
    check(4)   # captured (old stride) and replayed
    check(4)
    check(8)   # grows the arena: smaller slots
    check(4)   # must be re-captured, not replayed from the old arena
    check(4)
    check(1)
    check(8)
    g.close()


def test_candidates_one_not_positive_definite(gpmod):
    """One candidate of a batch whose matrix is not positive definite: its status says so, the
    others are unaffected (each candidate works in its own arena slot)."""
    rng = np.random.default_rng(9)
    X, y = _data(rng, 600, 2)
    X[311] = X[17]  # a duplicated input: with a noise variance below one ulp of the kernel
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise  # variance the pivot is exactly 0
    x_good, x_bad = np.log([1.0, 0.5, 0.2]), np.log([1.0, 0.5, 1e-13])
    g = gpmod.GP(2, simil, noise, X=X, Y=y)
    with pytest.raises(gpmod.FactorizeError):
        g.Observe(x_bad)
    want = (g.Observe(x_good), g.Gradient())
    xs = np.stack([x_good, x_bad, x_good])
    lmls, grads, status = g.observe_gradient_candidates(xs)
    assert list(status) == [0, 2, 0]
    assert np.isnan(lmls[1]) and not grads[1].any()
    for c in (0, 2):
        assert lmls[c] == want[0]
        np.testing.assert_array_equal(grads[c], want[1])
    g.close()


@pytest.mark.parametrize("n", [40, 600])
def test_candidates_leave_the_handle_alone_after_refused_ones(gpmod, n):
    """The candidates call works in an arena slot and puts the handle's own buffers and state back on the way out, also
    when some candidates fail: a good one, a refused one (non-finite x: GOGP_EARG = 1) and one whose matrix is not
    positive definite (GOGP_ENOTPD = 2).  Afterwards LML, Gradient (recomputed from the handle's own K^-1) and Produce
    are bit for bit what they were -- on the one-launch form (n <= 128) and on the general sweep.  Inputs 100 apart and a
    duplicated last one: at length 1 and noise 1e-13 K is the identity but for that pair, whose pivot is exactly 0."""
    rng = np.random.default_rng(n)
    X = 100.0 * np.arange(n, dtype=float)[:, None]
    X[-1] = X[-2]
    y = np.sin(X[:, 0] / 300.0) + 0.1 * rng.normal(size=n)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    x_own, x_good, x_bad = np.log([120.0, 120.0, 0.3]), np.log([150.0, 150.0, 0.2]), np.log([1.0, 1.0, 1e-13])
    x_refused = np.array([np.nan, 0.0, 0.0])
    Z = 100.0 * rng.uniform(0, n, (7, 1))
    g = gpmod.GP(1, simil, noise, X=X, Y=y)
    with pytest.raises(gpmod.FactorizeError):
        g.Observe(x_bad)
    want_good = (g.Observe(x_good), g.Gradient())
    g.Observe(x_own)
    before = (g.LML(), g.Gradient(), *g.Produce(Z))
    g.Observe(x_own)  # no cached gradient: Gradient() below reads the handle's own K^-1 and alpha again
    for rep in range(3):  # streams, then captured into a graph, then replayed
        lmls, grads, status = g.observe_gradient_candidates(np.stack([x_good, x_refused, x_bad]), strict=False)
        assert list(status) == [0, 1, 2]
        assert lmls[0] == want_good[0]
        np.testing.assert_array_equal(grads[0], want_good[1])
        assert np.isnan(lmls[1]) and np.isnan(lmls[2]) and not grads[1:].any()
        if rep == 0:
            after = (g.LML(), g.Gradient(), *g.Produce(Z))
            assert after[0] == before[0]
            for a, b in zip(after[1:], before[1:]):
                np.testing.assert_array_equal(a, b)
    after = (g.LML(), g.Gradient(), *g.Produce(Z))
    assert after[0] == before[0]
    for a, b in zip(after[1:], before[1:]):
        np.testing.assert_array_equal(a, b)
    g.close()


@pytest.mark.parametrize("graph", [1, 2])
def test_candidates_graph_follows_option_changes_between_replays(gpmod, graph):
    """A captured candidates graph is dropped by every option change (gogp_set_option), so the key it is replayed
    under holds no option.  Replayed, then super-panel width changed and changed back, then head_remaining 0 and 32
    (default 16) with replays in between: every LML and gradient bit for bit those of a graph = 0 handle with the
    same options."""
    rng = np.random.default_rng(700 + graph)
    n, D, k = 700, 3, 3
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    base = np.log([1.0, 0.7, 0.2])
    g, ref = gpmod.GP(D, simil, noise, X=X, Y=y), gpmod.GP(D, simil, noise, X=X, Y=y)
    g.set_option("graph", graph)
    ref.set_option("graph", 0)
    calls = [0]

    def replay(times):
        for _ in range(times):
            xs = base[None, :] + 0.02 * ((np.arange(k)[:, None] + calls[0]) % 5)
            calls[0] += 1
            lmls, grads, st = g.observe_gradient_candidates(xs)
            want = ref.observe_gradient_candidates(xs)
            assert list(st) == [0] * k
            np.testing.assert_array_equal(lmls, want[0])
            np.testing.assert_array_equal(grads, want[1])

    def set_both(name, value):
        g.set_option(name, value)
        ref.set_option(name, value)

    replay(3)  # seen, captured, replayed
    set_both("superpanel", 3)
    set_both("superpanel", 2)
    replay(3)
    set_both("head_remaining", 0)
    replay(3)
    set_both("head_remaining", 32)
    replay(3)
    assert not g.graph_info()[1]
    g.close()
    ref.close()


@pytest.mark.perf
def test_later_handles_as_fast_as_the_first(gpmod):
    """Stream sets are pooled (api.hip): a GP created after others were closed must run as
    fast as the first one.  With hipStreamDestroy + fresh streams every later handle of the
    process ran 55 % slower at N = 4096 (poor stream -> hardware-queue mapping)."""
    import time
    from gogp_amd import synth
    n, D = 4096, 8
    X, y = synth.make_inputs(n, D, 3)
    best = []
    for _ in range(3):
        g = gpmod.GP(D, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=X, Y=y)
        ts = []
        for k in range(4):
            t = time.perf_counter()
            g.Observe(synth.log_theta_cycle(D, k))
            g.Gradient()
            ts.append(time.perf_counter() - t)
        best.append(min(ts))
        g.close()
    assert max(best[1:]) <= 1.3 * best[0], best


@pytest.mark.parametrize("n", [50, 700])
def test_nan_inputs_behave_like_the_reference(gpmod, n):
    """NaN in an input row poisons a row/column of K: gonum's Cholesky fails and Absorb / Observe
    report "not positive definite" (gp/gp.go:228-230) -- here with the poisoned row as pivot.  NaN
    in an output only reaches alpha: LML and gradient are NaN, no error.  The handle recovers."""
    rng = np.random.default_rng(n)
    X, y = _data(rng, n, 2)
    x = np.log([1.0, 0.5, 0.1])
    Xn = X.copy()
    Xn[n // 2, 1] = np.nan
    g = gpmod.GP(2, kernel.Scaled(kernel.Normal), kernel.UniformNoise, X=Xn, Y=y)
    with pytest.raises(gpmod.FactorizeError):
        g.Observe(x)
    yn = y.copy()
    yn[3] = np.nan
    g.X, g.Y = X, yn
    assert math.isnan(g.Observe(x)) and np.isnan(g.Gradient()).all()
    g.X, g.Y = X, y
    assert np.isfinite(g.Observe(x)) and np.isfinite(g.Gradient()).all()
    g.close()


def test_handles_in_concurrent_host_threads(gpmod):
    """include/gogp_hip.h: calls on one handle are serialised by the caller, different handles
    may run concurrently.  Four handles driven from four host threads (ctypes releases the GIL)
    give bitwise the results of running them one after the other."""
    import threading

    def make(n, seed):
        r = np.random.default_rng(seed)
        return _data(r, n, 3)

    cases = [(1500, 1), (2100, 2), (900, 3), (1800, 4)]
    xs = [np.log([1.0, 0.5, 0.2]) + 0.01 * k for k in range(6)]

    def run(case, out):
        X, y = make(*case)
        g = gpmod.GP(3, kernel.Scaled(kernel.Matern32), kernel.UniformNoise, X=X, Y=y)
        for x in xs:
            out.append((g.Observe(x), g.Gradient().copy(), g.Produce(X[:5])[0].copy()))
        g.close()

    seq = [[] for _ in cases]
    for c, o in zip(cases, seq):
        run(c, o)
    par = [[] for _ in cases]
    ths = [threading.Thread(target=run, args=(c, o)) for c, o in zip(cases, par)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for a, b in zip(seq, par):
        assert len(a) == len(b) == len(xs)
        for (l0, g0, m0), (l1, g1, m1) in zip(a, b):
            assert l0 == l1
            np.testing.assert_array_equal(g0, g1)
            np.testing.assert_array_equal(m0, m1)


def test_out_of_memory_is_reported_and_recoverable(gpmod):
    """A problem that does not fit in HBM (N = 140000: three N x N fp64 buffers of 157 GB) fails
    with GOGP_ENOMEM, and the same handle then works on a small problem (the sticky HIP error of
    the failed hipMalloc must not leak into later calls)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(9)
    g = gpmod.GP(2, kernel.Scaled(kernel.Normal), kernel.UniformNoise)
    n = 140000
    g.X, g.Y = rng.uniform(0, 1, (n, 2)), rng.normal(size=n)
    x = np.log([1.0, 0.5, 0.1])
    with pytest.raises(gpmod.GogpError) as ei:
        g.Observe(x)
    assert ei.value.code == 5  # GOGP_ENOMEM
    X, y = _data(rng, 400, 2)
    g.X, g.Y = X, y
    o = FastOracle(2, kernel.Scaled(kernel.Normal), kernel.UniformNoise)
    o.set_data(X, y)
    lml, lml_o = g.Observe(x), o.Observe(x)
    assert abs(lml - lml_o) <= 1e-8 * max(1.0, abs(lml_o))
    np.testing.assert_allclose(g.Gradient(), o.Gradient(), rtol=1e-6, atol=1e-8)
    g.close()


def test_handle_reuse_across_sizes_and_call_orders(gpmod):
    """One GP value reused with growing and shrinking data, every call order the API
    allows (Observe -> Gradient twice, Observe -> Observe, Observe -> Absorb -> Produce,
    Produce right after an eager Observe while its gradient preparation is in flight)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(41)
    D = 2
    simil, noise = kernel.Scaled(kernel.Matern32), kernel.UniformNoise
    g = gpmod.GP(D, simil, noise)
    o = FastOracle(D, simil, noise)
    x = np.log([1.2, 0.4, 0.3])
    for n in (300, 900, 100, 513):
        X, y = _data(rng, n, D)
        g.X, g.Y = X, y
        o.set_data(X, y)
        lml_o = o.Observe(x)
        grad_o = o.Gradient()
        Z = rng.uniform(0, 1, (11, D))
        mu_o, sig_o = o.Produce(Z)
        # Observe -> Produce immediately (triangular inverse still running) -> Gradient x2
        assert abs(g.Observe(x) - lml_o) <= 1e-8 * abs(lml_o)
        mu, sig = g.Produce(Z)
        np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(sig, sig_o, rtol=1e-6, atol=1e-8)
        g1, g2 = g.Gradient(), g.Gradient()
        np.testing.assert_array_equal(g1, g2)
        assert np.abs(g1 - grad_o).max() <= 1e-6 * max(1.0, np.abs(grad_o).max())
        # Observe twice in a row (the first one's gradient preparation is abandoned)
        g.Observe(x + 0.05)
        assert abs(g.Observe(x) - lml_o) <= 1e-8 * abs(lml_o)
        # Absorb after Observe: no gradient any more, Produce still right
        g.ThetaSimil, g.ThetaNoise = list(np.exp(x[:2])), list(np.exp(x[2:]))
        g.Absorb(X, y)
        assert abs(g.LML() - lml_o) <= 1e-8 * abs(lml_o)
        with pytest.raises(gpmod.GogpError):
            g.Gradient()
        mu, sig = g.Produce(Z)
        np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8)


def test_absorb_big_then_observe_small_then_big(gpmod):
    """Regression (round-1 advisor finding): Absorb of a big data set sizes the N-dependent
    buffers without Y = L^-T; an Observe on small data then allocates Y; going back to the big
    data must not reuse that small Y with the big leading dimension."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(47)
    D = 2
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    Xb, yb = _data(rng, 1300, D)
    Xs, ys = _data(rng, 200, D)
    x = np.log([1.1, 0.45, 0.25])
    g = gpmod.GP(D, simil, noise)
    g.ThetaSimil, g.ThetaNoise = list(np.exp(x[:2])), list(np.exp(x[2:]))
    g.Absorb(Xb, yb)
    o = FastOracle(D, simil, noise)
    for X, y in ((Xs, ys), (Xb, yb), (Xs, ys), (Xb, yb)):
        g.X, g.Y = X, y
        o.set_data(X, y)
        lml_o, grad_o = o.Observe(x), o.Gradient()
        assert abs(g.Observe(x) - lml_o) <= 1e-8 * abs(lml_o)
        assert np.abs(g.Gradient() - grad_o).max() <= 1e-6 * max(1.0, np.abs(grad_o).max())
        np.testing.assert_allclose(g.Alpha, o.Alpha, rtol=1e-6, atol=1e-8)
    g.close()


def test_lazy_and_eager_paths_agree_bitwise_on_lml(gpmod):
    """eager=0 (triangular inverse on demand, backward substitution for alpha) and the
    fused sweep give the same LML bit for bit and the same gradient to rounding."""
    rng = np.random.default_rng(43)
    n, D = 1100, 3
    X, y = _data(rng, n, D)
    simil, noise = kernel.Scaled(kernel.Normal), kernel.UniformNoise
    x = np.log([0.9, 0.5, 0.15])
    a = gpmod.GP(D, simil, noise, X=X, Y=y)
    b = gpmod.GP(D, simil, noise, X=X, Y=y)
    b.set_option("eager", 0)
    c = gpmod.GP(D, simil, noise, X=X, Y=y)
    c.set_option("lookahead", 0)
    d = gpmod.GP(D, simil, noise, X=X, Y=y)
    d.set_option("superpanel", 1)
    la, lb, lc, ld_ = a.Observe(x), b.Observe(x), c.Observe(x), d.Observe(x)
    assert la == lb == lc
    assert abs(la - ld_) <= 1e-12 * abs(la)
    ga = a.Gradient()
    for other in (b, c, d):
        np.testing.assert_allclose(other.Gradient(), ga, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(b.Alpha, a.Alpha, rtol=1e-8, atol=1e-10)
    # run to run: bitwise reproducible (fixed-order reductions, no float atomics)
    assert a.Observe(x) == la
    np.testing.assert_array_equal(a.Gradient(), ga)


def test_two_handles_interleaved(gpmod):
    """Different GP values are independent (each owns its streams and buffers)."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(47)
    cases = []
    for D, simil in ((1, kernel.Scaled(kernel.Normal)), (4, kernel.Scaled(kernel.Matern52))):
        X, y = _data(rng, 400, D)
        g = gpmod.GP(D, simil, kernel.UniformNoise, X=X, Y=y)
        o = FastOracle(D, simil, kernel.UniformNoise)
        o.set_data(X, y)
        cases.append((g, o))
    x = np.log([1.0, 0.5, 0.2])
    lmls = [g.Observe(x) for g, _ in cases]  # both evaluations in flight before any gradient
    for (g, o), lml in zip(cases, lmls):
        assert abs(lml - o.Observe(x)) <= 1e-8 * abs(lml)
        go = o.Gradient()
        assert np.abs(g.Gradient() - go).max() <= 1e-6 * max(1.0, np.abs(go).max())


def test_ard_high_dimension(gpmod):
    """ARD-RBF at D=32 (the kernel of BASELINE config 5): P = 34 parameters."""
    from oracle.oracle import FastOracle
    rng = np.random.default_rng(53)
    n, D = 700, 32
    X, y = _data(rng, n, D)
    simil = kernel.Scaled(kernel.ARD(kernel.Normal, D))
    ls = math.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D))
    x = np.log(np.concatenate([[1.0], ls, [0.1]]))
    g = gpmod.GP(D, simil, kernel.UniformNoise, X=X, Y=y)
    o = FastOracle(D, simil, kernel.UniformNoise)
    o.set_data(X, y)
    lml, lml_o = g.Observe(x), o.Observe(x)
    assert abs(lml - lml_o) <= 1e-8 * abs(lml_o)
    gr, gr_o = g.Gradient(), o.Gradient()
    assert gr.shape == (34,)
    assert np.abs(gr - gr_o).max() <= 1e-6 * max(1.0, np.abs(gr_o).max())


def test_near_duplicate_inputs_with_default_noise(gpmod):
    """Nearly coincident inputs: K is close to singular and only the default
    ConstantNoise(1e-5) (gp/gp.go:43-48) keeps it positive definite."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(59)
    base = rng.uniform(0, 1, (30, 1))
    X = np.concatenate([base, base + 1e-7])
    y = np.sin(6 * X[:, 0])
    g = gpmod.GP(1, kernel.Scaled(kernel.Normal), None, X=X, Y=y)
    o = Oracle(1, kernel.Scaled(kernel.Normal), None)
    o.set_data(X, y)
    x = np.log([1.0, 0.3])
    try:
        lml_o = o.Observe(x)
    except Exception:
        with pytest.raises(gpmod.FactorizeError):
            g.Observe(x)
        return
    # cond(K) ~ 1e10: agree to cond * eps
    assert abs(g.Observe(x) - lml_o) <= 1e-4 * abs(lml_o)
