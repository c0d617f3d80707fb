"""Per-observation noise variances on the GPU (gogp_set_noise_variances, gogp_noise_variances_gradient, gogp_append_noisy,
gogp_remove) against the dense numpy reference of tests/noise_variances_ref.py, at the tolerances of
tests/test_gpu_parity.py: LML 1e-8 relative, vectors rtol 1e-6 / atol 1e-8, every gradient component -- dv included --
within 1e-6 of the largest.  Inputs and shapes: tests/noise_variances_ref.py (tests/test_noise_variances_cpu.py holds
every case to cond(K) <= 1e5).  After Absorb the gradient is refused as the reference refuses it (GOGP_ESTATE); every
other quantity is checked in both states."""
import ctypes

import numpy as np
import pytest

import append_ref as A
import basis_ref as BR
import loo_ref as LR
import multi_output_ref as MR
import noise_variances_ref as NV
from gogp_amd import _lib, kernel, optimize

pytestmark = pytest.mark.gpu

_REF = {}


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64))


def ref(fam, n, events=False):
    """The reference observed at the family's parameters: computed once, shared, read only."""
    key = (fam, n, events)
    if key not in _REF:
        D, simil, _ = NV.FAMILIES[fam]
        X, y, v, Z = NV.inputs(n, D)
        r = NV.Ref(D, simil, X, y, v, events=NV.EVENTS if events else None)
        r.observe(NV.log_theta(fam))
        r.Z = Z
        r.prod = {m: r.produce(Z[:m]) for m in NV.PRODUCE_M}
        _REF[key] = r
    return _REF[key]


def gp_of(fam, events=False, noise=NV.NOISE, tn=NV.TN, **kw):
    from gogp_amd.gp import GP
    D, simil, ts = NV.FAMILIES[fam]
    if events:
        simil = kernel.Events(simil, NV.EVENTS, 0)
    return GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, device=0, **kw)


def fit(g, fam, X, y, v, state):
    if state == "absorb":
        g.Absorb(X, y, v)
        return g.LML()
    g.X, g.Y = X, y
    g.SetNoiseVariances(v)
    return g.Observe(NV.log_theta(fam))


def snapshot(g, r, gradient):
    out = [np.array([g.LML()]), g.Alpha, g.NoiseVariancesGradient()]
    if gradient:
        out.append(g.Gradient())
    for m in NV.PRODUCE_M:
        out.extend(g.Produce(r.Z[:m]))
    return out


def check(g, r, tag, gradient=True):
    NV.assert_lml(g.LML(), r.lml, tag)
    NV.assert_vector(g.Alpha, r.alpha, tag)
    NV.assert_gradient(g.NoiseVariancesGradient(), r.dv, "%s dv" % (tag,))
    if gradient:
        NV.assert_gradient(g.Gradient(), r.grad, "%s gradient" % (tag,))
    else:
        from gogp_amd.gp import GogpError
        with pytest.raises(GogpError) as e:
            g.Gradient()
        assert e.value.code == _lib.GOGP_ESTATE
    for m in NV.PRODUCE_M:
        mu, sg = g.Produce(r.Z[:m])
        NV.assert_vector(mu, r.prod[m][0], (tag, "mu", m))
        NV.assert_vector(sg, r.prod[m][1], (tag, "sigma", m))


@pytest.mark.parametrize("state", ["absorb", "observe"])
@pytest.mark.parametrize("n", NV.SHAPES)
def test_shapes(n, state):
    r = ref(NV.MAIN, n)
    g = gp_of(NV.MAIN)
    lml = fit(g, NV.MAIN, r.X, r.y, r.v, state)
    assert lml == g.LML()
    np.testing.assert_array_equal(g.NoiseVariances, r.v)
    check(g, r, (n, state), gradient=state == "observe")
    first = snapshot(g, r, state == "observe")
    fit(g, NV.MAIN, r.X, r.y, r.v, state)  # a second round returns the same bits
    for a, b in zip(first, snapshot(g, r, state == "observe")):
        assert same_bits(a, b)
    g.close()


# ---- 1. zeros ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 129, 300, 700])
def test_zero_variances_give_the_bits_of_a_plain_handle(n):
    r = ref(NV.MAIN, n)
    plain = gp_of(NV.MAIN)
    if n <= 128:
        plain.set_option("tiny", 0)  # with variances the general sweep runs
    plain.X, plain.Y = r.X, r.y
    plain.Observe(NV.log_theta(NV.MAIN))
    g = gp_of(NV.MAIN)
    fit(g, NV.MAIN, r.X, r.y, np.zeros(n), "observe")
    for a, b in zip(snapshot(plain, r, True), snapshot(g, r, True)):
        assert same_bits(a, b)
    assert same_bits(plain.L, g.L)
    plain.close()
    g.close()


# ---- 2. constant v -----------------------------------------------------------------------------------------------------------
def test_constant_variances_match_a_larger_constant_noise():
    r = ref(NV.MAIN, 300)
    c = 0.7 * NV.S2
    g = gp_of(NV.MAIN)
    fit(g, NV.MAIN, r.X, r.y, np.full(300, c), "observe")
    k = gp_of(NV.MAIN, noise=kernel.ConstantNoise(float(np.sqrt(NV.S2 + c))), tn=None)
    k.X, k.Y = r.X, r.y
    k.Observe(np.log(NV.FAMILIES[NV.MAIN][2]))
    NV.assert_lml(g.LML(), k.LML(), "constant v")
    NV.assert_vector(g.Alpha, k.Alpha, "constant v")
    ns = len(NV.FAMILIES[NV.MAIN][2])
    NV.assert_gradient(g.Gradient()[:ns], k.Gradient()[:ns], "constant v gradient")
    NV.assert_gradient(g.NoiseVariancesGradient(), k.NoiseVariancesGradient(), "constant v dv")
    for a, b in zip(g.Produce(r.Z), k.Produce(r.Z)):
        NV.assert_vector(a, b, "constant v produce")
    g.close()
    k.close()


# ---- 3. the noise parameter's component ----------------------------------------------------------------------------------------
def test_noise_component_is_dnoise_times_the_sum_of_dv():
    r = ref(NV.MAIN, 300)
    g = gp_of(NV.MAIN)
    fit(g, NV.MAIN, r.X, r.y, r.v, "observe")
    grad, dv = g.Gradient(), g.NoiseVariancesGradient()
    want = 2.0 * NV.S2 * dv.sum()  # dnoise = d s2 / d log theta_n = 2 s2
    print("noise component %.9e, dnoise sum dv %.9e" % (grad[-1], want))
    assert abs(grad[-1] - want) <= 1e-6 * np.abs(grad).max()
    g.close()


# ---- 4. coverage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,events", [(f, False) for f in NV.FOUR] + [("matern52", True)],
                         ids=NV.FOUR + ["matern52-events"])
def test_kernel_families(fam, events):
    r = ref(fam, 300, events)
    g = gp_of(fam, events)
    fit(g, fam, r.X, r.y, r.v, "observe")
    check(g, r, (fam, events))
    g.close()


# ---- 5. the calls behind the factorisation ---------------------------------------------------------------------------------------
def test_downstream_calls_see_the_variances():
    fam = NV.MAIN
    D = NV.FAMILIES[fam][0]
    r = ref(fam, 300)
    g = gp_of(fam)
    fit(g, fam, r.X, r.y, r.v, "observe")
    mu_o, sg_o, lp_o, lg_o = LR.closed_form(r.K, r.y, r.dK)
    mu, sg, lp = g.LOO()
    NV.assert_vector(mu, mu_o, "LOO mu")
    NV.assert_vector(sg, sg_o, "LOO sigma")
    NV.assert_vector(lp, lp_o, "LOO logp")
    NV.assert_gradient(g.LOOGradient(), lg_o, "LOO gradient")
    Z = r.Z[:64]
    mu, cov = g.ProduceCovariance(Z)
    mu_o, cov_o = r.produce(Z, cov=True)
    NV.assert_vector(mu, mu_o, "covariance mu")
    NV.assert_vector(cov, cov_o, "covariance")
    Y = MR.outputs(r.X, 3, y0=r.y)
    g.SetOutputs(Y)
    np.testing.assert_array_equal(g.NoiseVariances, r.v)  # the setter leaves them alone
    total, per = g.MultiLML()
    _, lml_o, mg_o = MR.dense(r.K, Y, r.dK)
    np.testing.assert_allclose(per, lml_o, rtol=1e-8, atol=0)
    NV.assert_lml(total, lml_o.sum(), "multi total")
    NV.assert_gradient(g.MultiGradient(), mg_o, "multi gradient")
    H, _ = BR.case_basis(r.X, Z, 3 if D < 2 else 5)
    g.SetBasis(H)
    d = BR.dense(r.K, r.y, H, r.dK)
    NV.assert_lml(g.BasisLML(), d["lml"], "basis")
    NV.assert_gradient(g.BasisGradient(), d["grad"], "basis gradient")
    np.testing.assert_array_equal(g.NoiseVariances, r.v)
    g.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    from gogp_amd.gp import GogpError
    fam = NV.MAIN
    r = ref(fam, 300)
    x = NV.log_theta(fam)
    fresh = gp_of(fam)
    fresh.X, fresh.Y = r.X, r.y
    fresh.Observe(x)
    base = snapshot(fresh, r, True)
    g = gp_of(fam)
    g.X, g.Y = r.X, r.y
    g.Observe(x)
    # dv on a handle without variances: the derivative at v = 0; and the handle is left as found
    r0 = NV.Ref(NV.FAMILIES[fam][0], NV.FAMILIES[fam][1], r.X, r.y, None)
    r0.observe(x)
    before = (g.Gradient(), *g.Produce(r.Z))
    NV.assert_gradient(g.NoiseVariancesGradient(), r0.dv, "dv at v = 0")
    assert same_bits(g.NoiseVariancesGradient(), g.NoiseVariancesGradient())
    for a, b in zip(before, (g.Gradient(), *g.Produce(r.Z))):
        assert same_bits(a, b)
    assert not g.NoiseVariances.any()
    # a set drops the stored results until the next Observe
    g.SetNoiseVariances(r.v)
    for call in (g.Gradient, lambda: g.Produce(r.Z), g.LOO, g.NoiseVariancesGradient):
        with pytest.raises(GogpError) as e:
            call()
        assert e.value.code == _lib.GOGP_ESTATE
    g.Observe(x)
    check(g, r, "after set")
    before = (g.Gradient(), *g.Produce(r.Z))
    g.NoiseVariancesGradient()
    for a, b in zip(before, (g.Gradient(), *g.Produce(r.Z))):
        assert same_bits(a, b)
    # a clear restores a fresh handle's bits
    g.SetNoiseVariances(None)
    with pytest.raises(GogpError) as e:
        g.Gradient()
    assert e.value.code == _lib.GOGP_ESTATE
    g.Observe(x)
    for a, b in zip(base, snapshot(g, r, True)):
        assert same_bits(a, b)
    # set_data drops the variances ...
    g.SetNoiseVariances(r.v)
    g.X = r.X  # (the host layer uploads again at the next call)
    g.Observe(x)
    assert not g.NoiseVariances.any()
    for a, b in zip(base, snapshot(g, r, True)):
        assert same_bits(a, b)
    L = _lib.lib()
    g.SetNoiseVariances(r.v)
    assert L.gogp_set_data(g._h, dp(np.ascontiguousarray(r.X)), dp(r.y), 300) == _lib.GOGP_OK
    got = np.ones(300)
    assert L.gogp_get_noise_variances(g._h, dp(got)) == _lib.GOGP_OK and not got.any()
    # ... and so does the full form of Observe
    g.SetNoiseVariances(r.v)
    g.Observe(np.concatenate([x, r.X.reshape(-1), r.y]))
    assert not g.NoiseVariances.any()
    NV.assert_lml(g.LML(), r0.lml, "full form")
    # the other setters and gogp_set_factor leave them alone; the documented restore order
    src = gp_of(fam)
    src.Absorb(r.X, r.y, r.v)
    Lf, al = src.L, src.Alpha
    h = gp_of(fam)
    h.X, h.Y = r.X, r.y
    h.SetNoiseVariances(r.v)
    h.restore(Lf, al)
    np.testing.assert_array_equal(h.NoiseVariances, r.v)
    NV.assert_lml(h.LML(), r.lml, "restore")
    for m in (1, 64):
        mu, sg = h.Produce(r.Z[:m])
        NV.assert_vector(mu, r.prod[m][0], "restore mu")
        NV.assert_vector(sg, r.prod[m][1], "restore sigma")
    for q in (fresh, g, src, h):
        q.close()


# ---- 7. Append -------------------------------------------------------------------------------------------------------------------
def joined(n0, m, fam=NV.MAIN):
    D, simil, _ = NV.FAMILIES[fam]
    X, y, v, Z = NV.inputs(n0 + m, D, seed=23)
    return X, y, v, Z[:64]


def compare_joined(g, X, y, v, Z, tag, fam=NV.MAIN):
    D, simil, _ = NV.FAMILIES[fam]
    r = NV.Ref(D, simil, X, y, v)
    r.observe(NV.log_theta(fam))
    assert int(_lib.lib().gogp_n(g._h)) == len(y) == len(g.Y)
    np.testing.assert_array_equal(g.NoiseVariances, v)
    A.assert_state(g.LML(), g.Alpha, g.L, r.lml, r.alpha, r.L, tag)
    A.assert_produce(*g.Produce(Z), *r.produce(Z), tag)
    NV.assert_gradient(g.NoiseVariancesGradient(), r.dv, "%s dv" % (tag,))


@pytest.mark.parametrize("n0,m", [(1, 1), (255, 2), (256, 64), (300, 130)])
def test_append_matches_absorb_of_the_joined_data(n0, m):
    X, y, v, Z = joined(n0, m)
    g = gp_of(NV.MAIN)
    g.Absorb(X[:n0], y[:n0], v[:n0])
    g.Append(X[n0:], y[n0:], v[n0:])
    compare_joined(g, X, y, v, Z, (n0, m))
    g.close()


def test_append_variants():
    n0, m = 300, 20
    X, y, v, Z = joined(n0, m)
    # v2 = None on a handle with variances: zeros for the new rows
    g = gp_of(NV.MAIN)
    g.Absorb(X[:n0], y[:n0], v[:n0])
    g.Append(X[n0:], y[n0:])
    compare_joined(g, X, y, np.concatenate([v[:n0], np.zeros(m)]), Z, "v2 = None")
    g.close()
    # v2 on a handle without variances: zeros for the old rows
    g = gp_of(NV.MAIN)
    g.Absorb(X[:n0], y[:n0])
    g.Append(X[n0:], y[n0:], v[n0:])
    compare_joined(g, X, y, np.concatenate([np.zeros(n0), v[n0:]]), Z, "v2 on a plain handle")
    g.close()
    # the empty process absorbs the rows with their variances
    g = gp_of(NV.MAIN)
    g.Append(X[:n0], y[:n0], v[:n0])
    compare_joined(g, X[:n0], y[:n0], v[:n0], Z, "empty process")
    g.close()


def test_append_not_positive_definite_leaves_the_variances():
    """The recipe of tests/test_append_gpu.py::test_rollback_is_exact: a duplicate of x = 0 without any noise on either
    copy gives the pivot 1 - 1 = 0.  The same row with a variance of its own is then taken."""
    from gogp_amd.gp import GP, FactorizeError
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0], device=0)
    X0, y0, v0 = np.array([[0.0], [1.0]]), np.array([1.0, 0.0]), np.array([0.0, 0.5])
    g.Absorb(X0, y0, v0)
    Z = np.array([[0.25], [0.5], [1.5]])
    before = (np.array([g.LML()]), g.Alpha, g.L, g.NoiseVariances, *g.Produce(Z))
    np.testing.assert_array_equal(before[3], v0)
    with pytest.raises(FactorizeError) as ei:
        g.Append([[0.0]], [1.0], [0.0])
    assert ei.value.pivot == 2
    assert len(g.Y) == 2 and int(_lib.lib().gogp_n(g._h)) == 2
    for a, b in zip(before, (np.array([g.LML()]), g.Alpha, g.L, g.NoiseVariances, *g.Produce(Z))):
        assert same_bits(a, b)
    g.Append([[0.0]], [1.0], [0.25])
    r = NV.Ref(1, kernel.Normal, np.array([[0.0], [1.0], [0.0]]), [1.0, 0.0, 1.0], [0.0, 0.5, 0.25],
               noise=kernel.ConstantNoise(0.0))
    r.observe(np.log([1.0]))
    np.testing.assert_array_equal(g.NoiseVariances, r.v)
    NV.assert_lml(g.LML(), r.lml, "after the rollback")
    NV.assert_vector(g.Alpha, r.alpha, "after the rollback")
    g.close()


# ---- 8. Remove -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [[0], [151], list(range(3, 300, 9))], ids=["first", "middle", "33-rows"])
def test_remove_compacts_the_variances(idx):
    r = ref(NV.MAIN, 300)
    assert len(idx) in (1, 33)
    g = gp_of(NV.MAIN)
    g.Absorb(r.X, r.y, r.v)
    g.Remove(idx)
    keep = np.ones(300, bool)
    keep[idx] = False
    compare_joined(g, r.X[keep], r.y[keep], r.v[keep], r.Z[:64], ("remove", len(idx)))
    g.close()


# ---- 9. a sliding window ---------------------------------------------------------------------------------------------------------
def test_sliding_window():
    n, steps = 300, 5
    X, y, v, Z = joined(n, steps)
    g = gp_of(NV.MAIN)
    g.Absorb(X[:n], y[:n], v[:n])
    for k in range(steps):
        g.Remove([0])
        g.Append(X[n + k:n + k + 1], y[n + k:n + k + 1], v[n + k:n + k + 1])
    compare_joined(g, X[steps:], y[steps:], v[steps:], Z, "window")
    g.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gogp_amd.gp import GP, GogpError
    fam = NV.MAIN
    D, simil, ts = NV.FAMILIES[fam]
    r = ref(fam, 300)
    L = _lib.lib()
    x = NV.log_theta(fam)

    def refused(call, code, word):
        assert call() == code
        assert word in L.gogp_last_error(g._h), L.gogp_last_error(g._h)

    g = gp_of(fam)
    v, out = np.ascontiguousarray(r.v), np.zeros(300)
    # before the data is set
    refused(lambda: L.gogp_set_noise_variances(g._h, dp(v), 300), _lib.GOGP_ESTATE, b"no data")
    refused(lambda: L.gogp_get_noise_variances(g._h, dp(out)), _lib.GOGP_ESTATE, b"no data")
    refused(lambda: L.gogp_noise_variances_gradient(g._h, dp(out)), _lib.GOGP_ESTATE, b"no data")
    g.X, g.Y = r.X, r.y
    g._push_data()
    refused(lambda: L.gogp_noise_variances_gradient(g._h, dp(out)), _lib.GOGP_ESTATE, b"nothing absorbed")
    refused(lambda: L.gogp_set_noise_variances(g._h, dp(v), 299), _lib.GOGP_EARG, b"gogp_n")
    for bad in (-1e-12, np.nan, np.inf):
        w = v.copy()
        w[17] = bad
        refused(lambda: L.gogp_set_noise_variances(g._h, dp(w), 300), _lib.GOGP_EARG, b"finite")
    assert L.gogp_set_noise_variances(g._h, dp(v), 300) == _lib.GOGP_OK
    # the candidates path and the Laplace calls while variances are set
    with pytest.raises(GogpError) as e:
        g.observe_gradient_candidates(np.stack([x, x + 0.1]))
    assert e.value.code == _lib.GOGP_EARG and "noise variances" in str(e.value)
    with pytest.raises(GogpError) as e:
        g.LaplaceObserve(x, "poisson")
    assert e.value.code == _lib.GOGP_EARG and "noise variances" in str(e.value)
    # gradient_precision = 32, either way round
    refused(lambda: L.gogp_set_option(g._h, b"gradient_precision", 32), _lib.GOGP_EARG, b"noise variances")
    g.Observe(x)
    refused(lambda: L.gogp_append_noisy(g._h, dp(np.ascontiguousarray(r.X[:1])), dp(r.y[:1]), dp(np.array([-1.0])), 1),
            _lib.GOGP_EARG, b"finite")
    g.SetNoiseVariances(None)
    g.set_option("gradient_precision", 32)
    refused(lambda: L.gogp_set_noise_variances(g._h, dp(v), 300), _lib.GOGP_EARG, b"gradient_precision")
    refused(lambda: L.gogp_noise_variances_gradient(g._h, dp(out)), _lib.GOGP_EARG, b"gradient_precision")
    assert L.gogp_set_noise_variances(g._h, None, 0) == _lib.GOGP_OK  # clearing is always allowed
    g.close()
    # a precision = 32 handle
    g = GP(D, simil, NV.NOISE, ThetaSimil=ts, ThetaNoise=NV.TN, device=0, precision=32)
    g.Absorb(r.X, r.y)
    refused(lambda: L.gogp_set_noise_variances(g._h, dp(v), 300), _lib.GOGP_EARG, b"precision = 32")
    refused(lambda: L.gogp_noise_variances_gradient(g._h, dp(out)), _lib.GOGP_EARG, b"precision = 32")
    g.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    D, simil, ts = NV.FAMILIES[NV.MAIN]
    v = np.full(300, 0.01)

    def rank_fn(rk, lb):
        sh = ShardedGP(D, simil, NV.NOISE, device=0, grid=(1, 2), rank=rk, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        out = np.zeros(300)
        rcs, msgs = [], []
        for call in (lambda: L.gogp_set_noise_variances(sh._h, dp(v), 300),
                     lambda: L.gogp_noise_variances_gradient(sh._h, dp(out))):
            rcs.append(call())
            msgs.append(L.gogp_last_error(sh._h))
        sh.close()
        return rcs, msgs

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msgs in outs:
        assert rcs == [_lib.GOGP_EARG] * 2
        assert all(b"sharded" in m for m in msgs), msgs


# ---- 11. HeteroscedasticModel ------------------------------------------------------------------------------------------------------
def test_heteroscedastic_model():
    from gogp_amd.gp import GP, HeteroscedasticModel
    fam = NV.MAIN
    D, simil, ts = NV.FAMILIES[fam]
    n = 300
    rng = np.random.default_rng(4)
    X = rng.uniform(-2.0, 2.0, (n, D))
    G = np.zeros((n, 2))  # two instruments
    G[: n // 2, 0] = 1.0
    G[n // 2:, 1] = 1.0
    true_v = G @ np.array([0.2 * NV.S2, 3.0 * NV.S2])
    y = np.sin(X.sum(1)) + np.sqrt(NV.S2 + true_v) * rng.normal(size=n)
    g = GP(D, simil, NV.NOISE, X=X, Y=y, device=0)
    m = HeteroscedasticModel(g, G)
    r = NV.Ref(D, simil, X, y, None)
    x0 = np.concatenate([NV.log_theta(fam), np.log([NV.S2, NV.S2])])
    for x in (x0, x0 + np.array([0.2, -0.1, 0.15, -0.5, 0.7])):
        lml_o, grad_o = r.hetero(x, G)
        assert np.linalg.cond(r.K) <= NV.COND_MAX
        NV.assert_lml(m.Observe(x), lml_o, "hetero")
        NV.assert_gradient(m.Gradient(), grad_o, "hetero gradient")
        np.testing.assert_array_equal(g.NoiseVariances, np.exp(G @ x[-2:]))
    start = m.Observe(x0)
    res = optimize.lbfgs(m, x0, major_iterations=10)
    print("hetero objective: start %.9f, after %d iterations %.9f; v = %s (data made with %s)"
          % (start, res.iterations, res.lml, np.exp(res.x[-2:]), [0.2 * NV.S2, 3.0 * NV.S2]))
    assert res.lml > start
    with pytest.raises(ValueError):
        m.Observe(x0[:-1])
    with pytest.raises(ValueError):
        optimize.lbfgs(m, x0, major_iterations=2, line_search_candidates=4)  # the sequential drivers only
    g.close()
