"""Pin the CPU oracle against the reference's own known answers.

Mirrors gp/gp_test.go: TestProduce (gp_test.go:14-165) and TestElementalModel
(gp_test.go:173-269), case by case, with the reference's tolerances.  CPU only.
"""
import json
import math
import os

import numpy as np
import pytest

from gogp_amd import kernel
from oracle.oracle import FastOracle, Oracle


def _noise(spec):
    if spec["kind"] == "constant":
        return kernel.ConstantNoise(spec["std"])
    return kernel.UniformNoise


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "gp_test_known_answers.json")) as f:
        return json.load(f)


def test_produce_known_answers(known):
    # gp_test.go:133-162
    for c in known["produce"]:
        for cls in (Oracle, FastOracle):
            gp = cls(1, kernel.Normal, _noise(c["noise"]))
            gp.Absorb(np.array(c["x"], dtype=float).reshape(-1, 1), c["y"], c["theta_simil"])
            mu, sigma = gp.Produce(c["z"])
            assert len(mu) == len(c["mu"]) and len(sigma) == len(c["sigma"])
            for got, want in zip(mu, c["mu"]):
                assert abs(got - want) <= 1e-6, (c["name"], cls.__name__, mu)
            for got, want in zip(sigma, c["sigma"]):
                # 'self'/'two selves': variance - covariance rounds around 0; the
                # reference lets a NaN pass (math.Abs(NaN-x) > 1e-6 is false)
                if math.isnan(got):
                    assert want == 0
                    continue
                assert abs(got - want) <= 1e-6, (c["name"], cls.__name__, sigma)


def test_elemental_model_known_answers(known):
    # gp_test.go:231-267
    dx, eps = known["fd"]["dx"], known["fd"]["eps"]
    for c in known["elemental"]:
        gp = Oracle(1, kernel.Normal, _noise(c["noise"]))
        x = np.array(c["x"], dtype=float)
        ll = gp.Observe(x)
        dll = gp.Gradient()
        assert abs(ll - c["ll"]) < 1e-6, c["name"]
        assert len(dll) == len(x)
        for j in range(len(x)):
            xj = x.copy()
            xj[j] += dx
            llj = gp.Observe(xj)
            assert abs(dll[j] - (llj - ll) / dx) <= eps, (c["name"], j)
        # hyperparameters-only form, gp_test.go:254-267
        P = gp.ns + gp.nn
        n = (len(x) - P) // 2
        gp.set_data(x[P:P + n].reshape(-1, 1), x[P + n:])
        ll2 = gp.Observe(x[:P])
        dll2 = gp.Gradient()
        assert abs(ll2 - c["ll"]) < 1e-6
        assert len(dll2) == P
        np.testing.assert_allclose(dll2, dll[:P], rtol=1e-12, atol=1e-12)
        # the numpy twin agrees (hyperparameters-only)
        fo = FastOracle(1, kernel.Normal, _noise(c["noise"]))
        fo.set_data(x[P:P + n].reshape(-1, 1), x[P + n:])
        assert abs(fo.Observe(x[:P]) - c["ll"]) < 1e-6
        np.testing.assert_allclose(fo.Gradient(), dll[:P], rtol=1e-9, atol=1e-10)


def test_observe_leaves_argument_as_reference_does():
    # gp/gp.go:378-381,408-410: exp then log in place, <= 1 ulp drift
    gp = Oracle(1, kernel.Normal, kernel.UniformNoise)
    x = np.array([0.3, -1.2, 0.0, 1.0, 1.0, -1.0])
    x0 = x.copy()
    gp.Observe(x)
    np.testing.assert_allclose(x, x0, rtol=0, atol=4e-16)


def test_len_x_panics_like_reference():
    # gp/gp.go:398-400
    gp = Oracle(2, kernel.Normal, kernel.ConstantNoise(0.1))
    with pytest.raises(ValueError):
        gp.Observe(np.zeros(1 + 4))  # 4 leftovers, not a multiple of NDim+1 = 3


@pytest.mark.parametrize("name,simil,ns", [
    ("normal", kernel.Normal, 1),
    ("matern32", kernel.Matern32, 1),
    ("matern52", kernel.Matern52, 1),
    ("matern52tb", kernel.Matern52Textbook, 1),
    ("periodic", kernel.Periodic, 2),
    ("scaled_m32", kernel.Scaled(kernel.Matern32), 2),
    ("hyperpriors", kernel.Sum([kernel.Scaled(kernel.Matern52),
                                kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))],
                               order=[0, 2, 1, 3, 4]), 5),
])
def test_kernel_value_and_tape_gradient(name, simil, ns):
    """Closed-form partials == central finite differences of the value, and the
    value == the host kernel's Observe (kernel/kernel.go formulas)."""
    rng = np.random.default_rng(5)
    assert simil.NTheta() == ns
    gp = Oracle(1, simil, None)
    for _ in range(20):
        theta = rng.uniform(0.5, 2.0, ns)
        xa, xb = rng.normal(size=1), rng.normal(size=1)
        v, g = gp.simil(theta, xa, xb, with_grad=True)
        assert abs(v - simil.Observe(list(theta) + list(xa) + list(xb))) < 1e-14
        args = np.concatenate([theta, xa, xb])
        for i in range(len(args)):
            h = 1e-6
            ap, am = args.copy(), args.copy()
            ap[i] += h
            am[i] -= h
            fd = (simil.Observe(list(ap)) - simil.Observe(list(am))) / (2 * h)
            assert abs(fd - g[i]) < 1e-7, (name, i, fd, g[i])


def test_matern52_reference_coefficient_is_one():
    # kernel/kernel.go:91: 5/3 is integer division in Go
    d = 0.7
    want = (1 + kernel.SQRT5 * d + 1 * d * d) * math.exp(-kernel.SQRT5 * d)
    assert abs(kernel.Matern52.Observe([1.0, 0.0, d]) - want) < 1e-15
    tb = (1 + kernel.SQRT5 * d + 5.0 / 3.0 * d * d) * math.exp(-kernel.SQRT5 * d)
    assert abs(kernel.Matern52Textbook.Observe([1.0, 0.0, d]) - tb) < 1e-15


@pytest.mark.parametrize("simil,ndim,ntheta", [
    (kernel.Scaled(kernel.Normal), 3, 2),
    (kernel.Scaled(kernel.ARD(kernel.Normal, 3)), 3, 4),
    (kernel.Scaled(kernel.Matern32), 2, 2),
    (kernel.Scaled(kernel.Matern52), 2, 2),
    (kernel.Sum([kernel.Scaled(kernel.Matern52Textbook), kernel.Scaled(kernel.Periodic)]), 1, 5),
])
def test_fast_oracle_matches_faithful(simil, ndim, ntheta):
    """The W-matrix twin reproduces the faithful 1/2 tr(aa^T dK - K^-1 dK)."""
    rng = np.random.default_rng(11)
    n = 40
    X = rng.uniform(0, 1, (n, ndim))
    y = np.sin(X.sum(1) * 3) + 0.1 * rng.normal(size=n)
    noise = kernel.ScaledNoise(0.5)
    a = Oracle(ndim, simil, noise)
    assert simil.NTheta() == ntheta
    x = np.log(rng.uniform(0.5, 1.5, ntheta + 1))
    a.set_data(X, y)
    la = a.Observe(x)
    ga = a.Gradient()
    Z = rng.uniform(0, 1, (7, ndim))
    ma, sa = a.Produce(Z)
    for use_c in (True, False):  # C/OpenMP pair loops and the independent numpy path
        b = FastOracle(ndim, simil, noise, block=16, use_c=use_c)
        b.set_data(X, y)
        lb = b.Observe(x)
        assert abs(la - lb) < 1e-9 * max(1, abs(la))
        np.testing.assert_allclose(b.Gradient(), ga, rtol=1e-8, atol=1e-9)
        mb, sb = b.Produce(Z)
        np.testing.assert_allclose(mb, ma, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(sb, sa, rtol=1e-7, atol=1e-9)


def test_withobs_gradient_matches_fd():
    """Inputs/outputs gradient of the full form (gp/gp.go:118-129,488-493) on a
    D=2 Matern kernel against central differences."""
    rng = np.random.default_rng(3)
    n, D = 6, 2
    simil = kernel.Scaled(kernel.Matern52)
    gp = Oracle(D, simil, kernel.UniformNoise)
    x = np.concatenate([np.log([1.3, 0.8, 0.3]), rng.normal(size=n * D), rng.normal(size=n)])
    ll = gp.Observe(x)
    g = gp.Gradient()
    assert len(g) == len(x)
    for j in range(len(x)):
        h = 1e-6
        xp, xm = x.copy(), x.copy()
        xp[j] += h
        xm[j] -= h
        fd = (gp.Observe(xp) - gp.Observe(xm)) / (2 * h)
        assert abs(fd - g[j]) < 1e-6 * max(1.0, abs(fd)), j
    assert np.isfinite(ll)


def test_barebones_csv_config1(golden_dir):
    """BASELINE config 1 plumbing: tutorial/data/barebones.csv with the barebones
    kernel c*Matern32 + 0.01*UniformNoise (tutorial/barebones/kernel/kernel.go)."""
    data = np.loadtxt(os.path.join(golden_dir, "barebones.csv"), delimiter=",")
    X, y = data[:, :1], data[:, 1]
    y = (y - y.mean()) / y.std()  # tutorial/tutorial.go:78-86
    simil = kernel.Scaled(kernel.Matern32)
    noise = kernel.ScaledNoise(0.01)
    a, b = Oracle(1, simil, noise), FastOracle(1, simil, noise)
    a.set_data(X, y)
    b.set_data(X, y)
    x = np.zeros(3)
    la, lb = a.Observe(x), b.Observe(x)
    assert abs(la - lb) < 1e-9
    np.testing.assert_allclose(b.Gradient(), a.Gradient(), rtol=1e-8, atol=1e-9)


# ---------------------------------------------------------------------------
# committed oracle regression vectors (tests/golden/make_oracle_vectors.py): written by
# the numpy twin, re-derived here by the C restatements
# ---------------------------------------------------------------------------
def _vectors(golden_dir):
    with open(os.path.join(golden_dir, "oracle_vectors.json")) as f:
        return json.load(f)["vectors"]


def _vector_inputs(v):
    from gogp_amd import synth
    X, y = synth.make_inputs(v["n"], v["ndim"], v["seed"])
    Z = synth.make_test_points(v["m"], v["ndim"], v["seed"] + 1)
    # the generator itself is pinned: sums for every vector, full inputs for the small ones
    assert X.sum() == v["x_sum"] and y.sum() == v["y_sum"] and Z.sum() == v["z_sum"]
    if "X" in v:
        np.testing.assert_array_equal(X, np.array(v["X"]))
        np.testing.assert_array_equal(y, np.array(v["y"]))
        np.testing.assert_array_equal(Z, np.array(v["Z"]))
    return X, y, Z


def _assert_vector(v, lml, grad, mu, sigma, rtol):
    tag = (v["case"], v["n"])
    assert abs(lml - v["lml"]) <= rtol * max(1.0, abs(v["lml"])), tag
    g = np.array(v["grad"])
    assert np.abs(np.asarray(grad) - g).max() <= 100 * rtol * max(1.0, np.abs(g).max()), tag
    np.testing.assert_allclose(mu, v["mu"], rtol=1e-6, atol=1e-7, err_msg=str(tag))
    np.testing.assert_allclose(sigma, v["sigma"], rtol=1e-6, atol=1e-6, err_msg=str(tag))


def test_oracle_vectors_c_restatements(golden_dir):
    from cases import CASES
    cases = {c[0]: c for c in CASES}
    vectors = _vectors(golden_dir)
    assert len(vectors) == 5 * len(CASES)
    for v in vectors:
        _, D, simil, noise, _, _ = cases[v["case"]]
        X, y, Z = _vector_inputs(v)
        x = np.array(v["log_theta"])
        impls = [FastOracle(D, simil, noise)]            # C/OpenMP pair loops + LAPACK
        if v["n"] <= 64:
            impls.append(Oracle(D, simil, noise))        # faithful dense-dK algorithm
        for o in impls:
            o.set_data(X, y)
            lml = o.Observe(x)
            grad = o.Gradient()
            mu, sigma = o.Produce(Z)
            _assert_vector(v, lml, grad, mu, sigma, rtol=1e-9)


def test_oracle_constant_noise_with_parameter():
    """The anynoise noise kernel (tutorial/anynoise/kernel/kernel.go:26-35) in the oracle: one
    parameter, constant value; gradient by the reference's own finite-difference recipe
    (gp/gp_test.go:168-171,242-252) with a central difference, both oracle flavours agree."""
    import sys as _sys
    _sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from cases import ANYNOISE
    from oracle.oracle import FastOracle, Oracle
    name, D, simil, noise, ts, tn = ANYNOISE
    assert noise.NTheta() == 1 and noise.Observe([0.3, 1.0]) == pytest.approx(1e-5)
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (15, D))
    y = np.sin(4 * X[:, 0]) + 0.1 * rng.normal(size=15)
    x = np.log(np.array(ts + tn))
    o, f = Oracle(D, simil, noise), FastOracle(D, simil, noise)
    o.set_data(X, y)
    f.set_data(X, y)
    ll = o.Observe(x)
    g = o.Gradient()
    assert abs(f.Observe(x) - ll) < 1e-9
    np.testing.assert_allclose(f.Gradient(), g, rtol=1e-7, atol=1e-9)
    assert g[2] == 0.0
    # K has cond ~ 1e5 / 1e-5 here: a forward difference with the reference's dx = 1e-8 is
    # dominated by rounding, so use a central difference and a relative tolerance
    for j in range(3):
        xp, xm = x.copy(), x.copy()
        xp[j] += 1e-5
        xm[j] -= 1e-5
        fd = (o.Observe(xp) - o.Observe(xm)) / 2e-5
        assert abs(g[j] - fd) <= 1e-4 * max(1.0, abs(g[j])), (j, g[j], fd)


# ---------------------------------------------------------------------------
# the record behind tests/test_schedule_regimes_gpu.py (tests/golden/make_schedule_regimes.py)
# ---------------------------------------------------------------------------
def test_schedule_regimes_record_covers_the_case_table(golden_dir):
    """schedule_regimes.json holds exactly the cases of tests/cases.py, every one with a usable tolerance record and
    the condition the per-component gradient check rests on; the generator's inputs of every case reproduce the
    recorded checksums, and the oracle on the smallest case the recorded LML and gradient; the thresholds the case
    table straddles are still the ones the library's source states."""
    import importlib.util
    from cases import REGIME_CASES, REGIME_FAMILIES, REGIME_SIZES, REGIME_THRESHOLDS, regime_inputs
    with open(os.path.join(golden_dir, "schedule_regimes.json")) as f:
        cases = json.load(f)["cases"]
    assert [(c["family"], c["n"]) for c in cases] == REGIME_CASES
    spec = importlib.util.spec_from_file_location("make_schedule_regimes",
                                                  os.path.join(golden_dir, "make_schedule_regimes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for c in cases:
        assert c["n"] in REGIME_SIZES and c["n"] % 256 != 0
        again = gen.checksums(c["family"], c["n"])
        assert all(c[k] == v for k, v in again.items()), (c["family"], c["n"])
        assert len(c["grad_disagreement"]) == len(c["grad"]) == len(c["log_theta"])
        assert 0 < c["lml_disagreement"] < 1e-11 and 0 < min(c["grad_disagreement"])
        assert max(c["grad_disagreement"]) < 1e-7
        assert c["min_component_ratio"] >= gen.MIN_COMPONENT_RATIO and c["cond_diag"] < 1e3
        assert 0 < c["rho_ref"] < 0.125   # min(1, 8 rho_ref) binds: the GPU factor is held to LAPACK's, not to 1
    c = min(cases, key=lambda c: (c["n"], c["ndim"]))
    D, simil, noise = REGIME_FAMILIES[c["family"]][:3]
    X, y, _, x = regime_inputs(c["family"], c["n"])
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    assert abs(o.Observe(x) - c["lml"]) <= 1e-11 * abs(c["lml"])
    np.testing.assert_allclose(o.Gradient(), c["grad"], rtol=1e-7, atol=0)
    src = os.path.join(os.path.dirname(os.path.dirname(golden_dir)), "gogp_amd", "csrc")
    with open(os.path.join(src, "api.hip")) as f:
        api = f.read()
    with open(os.path.join(src, "handle.h")) as f:
        handle = f.read()
    t = REGIME_THRESHOLDS
    assert "int head_remaining = %d;" % (t["superpanel_head"] // 256) in handle
    assert "h->npad <= %d ? 1 : 0" % t["chain_prio"] in api
    assert "(h->npad <= %d || !eager) ? 2 : 0" % t["chain_split"] in api
    assert "GRAPH_EXPLICIT_MAX_NPAD = %d;" % t["graph_explicit"] in api
    assert "(npad <= %d || " % t["kinv_fused"] in api
