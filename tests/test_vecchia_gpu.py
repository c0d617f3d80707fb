"""Vecchia's approximation on the GPU through the C ABI (GP.SetVecchia / VecchiaObserve / VecchiaTerms / VecchiaGradient /
VecchiaProduce, VecchiaModel), against the reference's float64 results recorded in tests/golden/vecchia.json
(tools/make_vecchia_golden.py; the inputs come from seeds: vecchia_ref.golden_problem), the dense path of the same build and
central differences of the value itself.  Every figure is printed before it is asserted (-s).  The N x 3 terms are the
one quantity the file does not hold (it would be half a megabyte): the float64 reference recomputes them here, once per
case and without the gradient, and the file holds their magnitudes and the reference's own differences.

Tolerance against the reference: 8 x its own float64-minus-long-double difference (the factor of the CG tests) -- per
quantity the largest over the golden cases of (difference / the quantity's largest magnitude), times the magnitude in
the case at hand.  The golden blocks are well conditioned (tests/test_vecchia_cpu.py asserts that no pivot fails), so this
is a statement about rounding.  The exact cases are held to the dense Observe + Gradient with the same tolerance: their
golden differences come from factoring the same 64 x 64 matrix.  Only the dense Produce at all rows, which has no golden
counterpart, gets the floor cond N u of the CG tests.  Every device result is computed once per case and shared, read
only."""
import ctypes
import json
import os

import numpy as np
import pytest

import grad_reduce_ref as G
import gram_ref as R
import vecchia_ref as V
from gogp_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "vecchia.json")) as _f:
    GOLD = json.load(_f)["cases"]
FACTOR = 8.0
U = 2.0 ** -53
EA, ES, OK, ENOTPD = _lib.GOGP_EARG, _lib.GOGP_ESTATE, _lib.GOGP_OK, _lib.GOGP_ENOTPD
REFERENCE = [n for n in V.GOLDEN if not n.startswith("exact")]
EXACT = [n for n in V.GOLDEN if n.startswith("exact")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dp(a):
    return a.ctypes.data_as(_lib._dp)


def _norms(name):
    """The magnitudes the quantities of a case are judged by (mu in units of y: it is a forecast of y)."""
    c, p = GOLD[name], _problem(name)
    t = c["terms_norm"]
    ymax = float(np.abs(p["y"]).max())
    n = dict(value=abs(c["value"]), mu_t=max(t[0], ymax), s_t=t[1], logp_t=t[2], grad=float(np.abs(c["grad"]).max()))
    if "mu" in c:
        n.update(mu=max(float(np.abs(c["mu"]).max()), ymax), sigma=float(np.abs(c["sigma"]).max()))
    return n


_P, _RUN, _SHARE, _TERMS = {}, {}, {}, {}


def _problem(name):
    if name not in _P:
        _P[name] = V.golden_problem(name)
    return _P[name]


def share():
    """Per quantity the reference's largest relative float64-minus-long-double difference over the golden cases."""
    if not _SHARE:
        for name, c in GOLD.items():
            n = _norms(name)
            d = dict(value=c["value_diff"], mu_t=c["terms_diff"][0], s_t=c["terms_diff"][1], logp_t=c["terms_diff"][2],
                     grad=max(c["grad_diff"]))
            if "mu" in c:
                d.update(mu=c["mu_diff"], sigma=c["sigma_diff"])
            for q, v in d.items():
                _SHARE[q] = max(_SHARE.get(q, 0.0), v / n[q])
        assert all(0 < v < 1e-10 for v in _SHARE.values()), _SHARE
    return _SHARE


def _reference_terms(name):
    """The float64 reference's terms of a case (not recorded: the module docstring), held to the file by their sum."""
    if name not in _TERMS:
        p = _problem(name)
        a = V.observe(p["kp"], p["X"], p["y"], p["v"], p["t"], "f64", grad=False)
        assert not a["failed"] and abs(a["value"] - GOLD[name]["value"]) <= 1e-9 * abs(GOLD[name]["value"])
        _TERMS[name] = a["terms"]
    return _TERMS[name]


def tol(name, q):
    return FACTOR * share()[q] * _norms(name)[q]


def _gp(p, **kw):
    from gogp_amd.gp import GP
    return GP(p["D"], p["simil"], p["noise"], ThetaSimil=list(p["ts"]), ThetaNoise=list(p["tn"]), device=0, **kw)


def _observed(name):
    """One process per golden case: value, terms, gradient, mu and sigma of the test points; shared, read only."""
    if name not in _RUN:
        p = _problem(name)
        g = _gp(p)
        g.SetVecchia(p["X"], p["y"], p["t"], p["v"])
        value = g.VecchiaObserve(p["x"])
        mu_t, s_t, logp_t = g.VecchiaTerms()
        grad = g.VecchiaGradient()
        mu, sigma = g.VecchiaProduce(p["Z"], p["tz"])
        g.close()
        r = dict(value=value, mu_t=mu_t, s_t=s_t, logp_t=logp_t, grad=grad, mu=mu, sigma=sigma)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _RUN[name] = r
    return _RUN[name]


def _judge(name, r, quantities):
    c = GOLD[name]
    t = _reference_terms(name)
    want = dict(value=c["value"], mu_t=t[:, 0], s_t=t[:, 1], logp_t=t[:, 2], grad=np.array(c["grad"]),
                mu=np.array(c.get("mu", [])), sigma=np.array(c.get("sigma", [])))
    ok = True
    for q in quantities:
        err = float(np.abs(np.asarray(r[q]) - want[q]).max())
        print("%s %-6s |err| %.3g, allowed %.3g" % (name, q, err, tol(name, q)))
        ok = ok and err <= tol(name, q)
    return ok


@pytest.mark.parametrize("name", REFERENCE)
def test_against_the_reference(name):
    """LML, all terms, the gradient with the noise parameter's component and, where the file records them (N = 200), mu
    and sigma of 65 test points."""
    r = _observed(name)
    assert len(r["grad"]) == len(_problem(name)["x"])
    assert _judge(name, r, ("value", "mu_t", "s_t", "logp_t", "grad") + (("mu", "sigma") if "mu" in GOLD[name] else ()))
    assert abs(r["value"] - float(np.sum(r["logp_t"]))) <= 1e-9 * abs(r["value"])


@pytest.mark.parametrize("name", EXACT)
def test_all_earlier_rows_are_exact(name):
    """N = 64, c(i) = every earlier row: value and gradient against the reference and, with the same golden-derived
    tolerance, against the dense Observe + Gradient of the same build."""
    p, r = _problem(name), _observed(name)
    assert _judge(name, r, ("value", "mu_t", "s_t", "logp_t", "grad"))
    d = _gp(p)
    d.Absorb(p["X"], p["y"])
    dl, dg = d.Observe(p["x"]), d.Gradient()
    d.close()
    print("%s: |value - dense| %.3g (allowed %.3g), |grad - dense| %.3g (allowed %.3g)"
          % (name, abs(r["value"] - dl), tol(name, "value"), np.abs(r["grad"] - dg).max(), tol(name, "grad")))
    assert abs(r["value"] - dl) <= tol(name, "value")
    assert np.abs(r["grad"] - dg).max() <= tol(name, "grad")


def test_zero_variances_are_no_variances():
    """v = 0 and v = None: noise_var + 0 is noise_var, so every bit agrees."""
    name = "nearest-N200-m7"
    p, r = _problem(name), _observed(name)
    g = _gp(p)
    g.SetVecchia(p["X"], p["y"], p["t"], np.zeros(p["N"]))
    value = g.VecchiaObserve(p["x"])
    terms, grad = g.VecchiaTerms(), g.VecchiaGradient()
    g.close()
    assert value == r["value"] and np.array_equal(bits(grad), bits(r["grad"]))
    assert np.array_equal(bits(terms[0]), bits(r["mu_t"])) and np.array_equal(bits(terms[2]), bits(r["logp_t"]))


@pytest.mark.parametrize("name", ["nearest-N200-m31", "previous-N200-m7"])
def test_gradient_is_the_derivative_of_the_value(name):
    """Central differences of VecchiaObserve itself at h and 2 h.  Their own error: truncation, estimated from the two
    step sizes (the difference at h errs by a third of |fd(h) - fd(2 h)| when the h^2 term leads; the whole difference is
    allowed), and the rounding of two values, each within the reference tolerance of the value, divided by 2 h."""
    p, r = _problem(name), _observed(name)
    g = _gp(p)
    g.SetVecchia(p["X"], p["y"], p["t"], p["v"])
    h = 1e-3
    worst = 0.0
    for k in range(len(p["x"])):
        fd = []
        for step in (h, 2 * h):
            e = np.zeros(len(p["x"]))
            e[k] = step
            fd.append((g.VecchiaObserve(p["x"] + e) - g.VecchiaObserve(p["x"] - e)) / (2 * step))
        allowed = abs(fd[0] - fd[1]) + 2 * tol(name, "value") / (2 * h)
        err = abs(fd[0] - r["grad"][k])
        print("%s component %d: gradient %.9g, differences %.9g / %.9g, |err| %.3g, allowed %.3g"
              % (name, k, r["grad"][k], fd[0], fd[1], err, allowed))
        worst = max(worst, err / allowed)
    g.close()
    assert worst <= 1.0


def test_produce():
    """One test point and 65; sigma = NULL; c* = all rows at N = 63 against the dense Produce."""
    name = "nearest-N200-m31"
    p, r = _problem(name), _observed(name)
    g = _gp(p)
    g.SetVecchia(p["X"], p["y"], p["t"], p["v"])
    g.VecchiaObserve(p["x"])
    mu1, sg1 = g.VecchiaProduce(p["Z"][:1], p["tz"][:1])
    mu, none = g.VecchiaProduce(p["Z"], p["tz"], sigma=False)
    assert none is None and np.array_equal(bits(mu), bits(r["mu"]))
    assert mu1[0] == r["mu"][0] and sg1[0] == r["sigma"][0], "a test point alone has the bits it has among 65"
    e = np.zeros((0, p["D"]))
    assert g.VecchiaProduce(e, np.zeros((0, p["m"]), np.int32))[0].shape == (0,)
    for cols in (p["m"] - 1, p["m"] + 1):  # a table of another m would be read past its end, or mis-strided
        with pytest.raises(ValueError):
            g.VecchiaProduce(p["Z"], np.ascontiguousarray(np.resize(p["tz"], (len(p["Z"]), cols))))
    g.close()
    # all rows: the exact posterior
    N = 63
    X, y = p["X"][:N], p["y"][:N]
    tz = np.tile(np.arange(N, dtype=np.int32), (len(p["Z"]), 1))
    g = _gp(p)
    t = np.full((N, N), -1, np.int32)  # m = 63 columns, as the test points' table has
    t[:, :N - 1] = V.all_earlier(N)
    g.SetVecchia(X, y, t)
    g.VecchiaObserve(p["x"])
    mu, sigma = g.VecchiaProduce(p["Z"], tz)
    g.Absorb(X, y)
    dmu, dsigma = g.Produce(p["Z"])
    g.close()
    K = np.asarray(R.pair_values(p["kp"], X, X, "f64")[0]) + p["kp"].noise_var * np.eye(N)
    floor = float(np.linalg.cond(K)) * N * U
    ymax = float(np.abs(y).max())
    print("all rows: cond %.3g, |mu - dense| %.3g, |sigma - dense| %.3g, allowed %.3g x size"
          % (floor / (N * U), np.abs(mu - dmu).max(), np.abs(sigma - dsigma).max(), 2 * floor))
    # both sides carry the conditioning; sigma = sqrt(prior - q) loses what the subtraction cancels: judged through sigma^2
    assert np.abs(mu - dmu).max() <= 2 * floor * ymax
    assert np.abs(sigma ** 2 - np.asarray(dsigma) ** 2).max() <= 2 * floor * R.prior_values(p["kp"])


def test_terms_are_one_step_ahead_forecasts():
    """previous(n, m): term i is the dense Produce of x[i] fitted on the rows i - m .. i - 1 -- mu_i its mean, s_i^2 its
    latent variance plus the noise.  Both sides factor the same m x m matrix (cond <= 1 + sum c / noise_var ~ 1e4 at
    m = 31): cond m u is below 1e-10 of the size, 1e-9 is allowed."""
    name = "previous-N200-m31"
    p, r = _problem(name), _observed(name)
    m, nv = p["m"], p["kp"].noise_var
    for i in (31, 100, 199):
        d = _gp(p)
        d.Absorb(p["X"][i - m:i], p["y"][i - m:i])
        d.Observe(p["x"])
        mu, sigma = d.Produce(p["X"][i:i + 1])
        d.close()
        print("forecast %d: mu %.12g against %.12g, s %.12g against %.12g" % (i, r["mu_t"][i], mu[0], r["s_t"][i],
                                                                              np.sqrt(sigma[0] ** 2 + nv)))
        assert abs(r["mu_t"][i] - mu[0]) <= 1e-9 * np.abs(p["y"]).max()
        assert abs(r["s_t"][i] ** 2 - (sigma[0] ** 2 + nv)) <= 1e-9 * (R.prior_values(p["kp"]) + nv)


def test_contracts():
    """The handle's other state is left as found; identical calls give identical bits; every error code."""
    from gogp_amd.gp import FactorizeError, GogpError
    name = "nearest-N200-m7"
    p, r = _problem(name), _observed(name)
    L = _lib.lib()
    N, m, D = p["N"], p["m"], p["D"]
    g = _gp(p)
    Xd, yd = p["X"][:50], p["y"][:50]
    g.Absorb(Xd, yd)
    before = (g.Observe(p["x"]), g.Gradient(), g.Produce(p["Z"][:4]))
    g.SetVecchia(p["X"], p["y"], p["t"], p["v"])
    a = (g.VecchiaObserve(p["x"]), g.VecchiaTerms(), g.VecchiaGradient(), g.VecchiaProduce(p["Z"], p["tz"]))
    after = (g.Observe(p["x"]), g.Gradient(), g.Produce(p["Z"][:4]))
    b = (g.VecchiaObserve(p["x"]), g.VecchiaTerms(), g.VecchiaGradient(), g.VecchiaProduce(p["Z"], p["tz"]))
    assert before[0] == after[0] and np.array_equal(bits(before[1]), bits(after[1]))
    assert all(np.array_equal(bits(u), bits(w)) for u, w in zip(before[2], after[2])), "the dense state moved"
    assert a[0] == b[0] == r["value"] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[2]), bits(r["grad"]))
    assert all(np.array_equal(bits(u), bits(w)) for u, w in zip(a[1] + a[3], b[1] + b[3])), "identical calls differ"
    # the C calls' refusals
    X, y, t, x = np.ascontiguousarray(p["X"]), p["y"].copy(), np.ascontiguousarray(p["t"]), p["x"].copy()
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out, val = np.zeros(3 * N), ctypes.c_double(0.0)
    assert L.gogp_vecchia_observe(g._h, _dp(x), x.size - 1, ctypes.byref(val), None) == EA, "len"
    assert L.gogp_vecchia_observe(g._h, None, x.size, ctypes.byref(val), None) == EA
    assert L.gogp_vecchia_observe(g._h, _dp(x), x.size, None, None) == EA
    xn = x.copy()
    xn[0] = np.nan
    assert L.gogp_vecchia_observe(g._h, _dp(xn), x.size, ctypes.byref(val), None) == EA
    assert L.gogp_vecchia_gradient(g._h, _dp(out), x.size + 1) == EA and L.gogp_vecchia_gradient(g._h, None, x.size) == EA
    bad = t.copy()
    bad[17, 0] = 17
    assert L.gogp_vecchia_set_data(g._h, _dp(X), _dp(y), None, N, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m) == EA
    assert b"row 17" in L.gogp_last_error(g._h)
    assert L.gogp_vecchia_set_data(g._h, _dp(X), _dp(y), None, N, tp, 64) == EA
    assert L.gogp_vecchia_set_data(g._h, _dp(X), None, None, N, tp, m) == EA
    yn = y.copy()
    yn[3] = np.inf
    assert L.gogp_vecchia_set_data(g._h, _dp(X), _dp(yn), None, N, tp, m) == EA
    vn = np.full(N, -1.0)
    assert L.gogp_vecchia_set_data(g._h, _dp(X), _dp(y), _dp(vn), N, tp, m) == EA
    assert g.VecchiaObserve(p["x"]) == r["value"], "a refused set_data leaves the data in place"
    tzb = np.ascontiguousarray(p["tz"]).copy()
    tzb[5, 1] = N
    Z = np.ascontiguousarray(p["Z"])
    assert L.gogp_vecchia_produce(g._h, _dp(Z), len(Z), tzb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(out), None) == EA
    assert b"row 5" in L.gogp_last_error(g._h)
    assert L.gogp_vecchia_produce(g._h, _dp(Z), len(Z), None, _dp(out), None) == EA
    assert L.gogp_vecchia_produce(g._h, None, 0, None, None, None) == OK
    # event discounts: refused by name, and accepted again once cleared
    ev = np.array([0.0, 1.0, 0.5])
    assert L.gogp_set_events(g._h, _dp(ev), 1, 0) == OK
    assert L.gogp_vecchia_observe(g._h, _dp(x), x.size, ctypes.byref(val), None) == EA and b"event" in L.gogp_last_error(g._h)
    assert L.gogp_vecchia_set_data(g._h, _dp(X), _dp(y), None, N, tp, m) == EA
    assert L.gogp_vecchia_gradient(g._h, _dp(out), x.size) == EA
    assert L.gogp_vecchia_produce(g._h, _dp(Z), len(Z), p["tz"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(out), None) == EA
    assert L.gogp_set_events(g._h, None, 0, 0) == OK
    assert g.VecchiaObserve(p["x"]) == r["value"]
    # the order of the calls
    g.SetVecchia(p["X"], p["y"], p["t"], p["v"])
    assert L.gogp_vecchia_gradient(g._h, _dp(out), x.size) == ES, "gradient before observe"
    assert L.gogp_vecchia_produce(g._h, _dp(Z), len(Z), p["tz"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(out), None) == ES
    g.SetVecchia(None, None, None)
    assert L.gogp_vecchia_observe(g._h, _dp(x), x.size, ctypes.byref(val), None) == ES
    with pytest.raises(GogpError) as e:
        g.VecchiaTerms()
    assert e.value.code == ES
    with pytest.raises(ValueError):
        g.SetVecchia(p["X"], p["y"][:-1], p["t"])
    with pytest.raises(ValueError):
        g.SetVecchia(p["X"], p["y"], p["t"][:-1])
    g.close()
    g32 = _gp(p, precision=32)
    with pytest.raises(GogpError) as e:
        g32.SetVecchia(p["X"], p["y"], p["t"])
    assert e.value.code == EA and "precision = 32" in str(e.value)
    assert L.gogp_vecchia_observe(g32._h, _dp(x), x.size, ctypes.byref(val), None) == EA
    g32.close()
    # GOGP_ENOTPD carries the row: rows 5 and 9 coincide, no noise, Normal kernel at scale 1 (tests/test_vecchia_kernel.py)
    from gogp_amd import kernel as GK
    from gogp_amd.gp import GP
    X2, y2, _ = V.inputs(3, 40, 2)
    X2 = X2.copy()
    X2[9] = X2[5]
    t2 = np.full((40, 2), -1, np.int32)
    t2[9], t2[20], t2[30] = (5, -1), (5, 9), (3, 4)
    g0 = GP(2, GK.Normal, GK.ConstantNoise(0.0), ThetaSimil=[2.0], device=0)
    g0.SetVecchia(X2, y2, t2)
    with pytest.raises(FactorizeError) as e:
        g0.VecchiaObserve(np.log([2.0]))
    assert L.gogp_notpd_index(g0._h) == 9 and "row 9" in str(e.value)
    mu_t, s_t, logp_t = g0.VecchiaTerms()
    assert np.isnan(mu_t[[9, 20]]).all() and np.isfinite(np.delete(logp_t, [9, 20])).all()
    assert L.gogp_vecchia_gradient(g0._h, _dp(out), 1) == ES, "a failed observe leaves nothing to differentiate"
    g0.close()


def test_sharded_handles_are_refused():
    import loopback
    from gogp_amd.sharded import ShardedGP
    p = _problem("nearest-N200-m7")
    X, y, t, x = np.ascontiguousarray(p["X"]), p["y"].copy(), np.ascontiguousarray(p["t"]), p["x"].copy()
    Z, tz = np.ascontiguousarray(p["Z"]), np.ascontiguousarray(p["tz"])

    def rank_fn(r, lb):
        sh = ShardedGP(p["D"], p["simil"], p["noise"], device=0, grid=(1, 2), rank=r, world=2, exchange=lb.exchange,
                       allreduce=lb.allreduce)
        L = _lib.lib()
        out, val = np.zeros(3 * p["N"]), ctypes.c_double(0.0)
        i32 = ctypes.POINTER(ctypes.c_int32)
        rcs, msgs = [], []
        for call in (lambda: L.gogp_vecchia_set_data(sh._h, _dp(X), _dp(y), None, p["N"], t.ctypes.data_as(i32), p["m"]),
                     lambda: L.gogp_vecchia_observe(sh._h, _dp(x), x.size, ctypes.byref(val), None),
                     lambda: L.gogp_vecchia_gradient(sh._h, _dp(out), x.size),
                     lambda: L.gogp_vecchia_produce(sh._h, _dp(Z), len(Z), tz.ctypes.data_as(i32), _dp(out), None)):
            rcs.append(call())
            msgs.append(L.gogp_last_error(sh._h))
        sh.close()
        return rcs, msgs

    outs, _ = loopback.run_ranks(2, rank_fn)
    for rcs, msgs in outs:
        assert rcs == [EA] * 4 and all(b"sharded" in m for m in msgs), (rcs, msgs)


def test_model_under_lbfgs():
    """VecchiaModel as an objective: a few L-BFGS iterations on N = 500 increase the value."""
    from gogp_amd import optimize, vecchia
    from gogp_amd.gp import VecchiaModel
    p = _problem("nearest-N1000-m7")
    X, y = p["X"][:500], p["y"][:500]
    g = _gp(p)
    g.SetVecchia(X, y, vecchia.nearest(X, 15))
    model = VecchiaModel(g)
    x0 = p["x"] + 0.3
    v0 = model.Observe(x0)
    g0 = model.Gradient()
    res = optimize.lbfgs(model, x0, major_iterations=5)
    v1 = model.Observe(np.asarray(res.x, dtype=float))
    g.close()
    print("VecchiaModel: value %.6f -> %.6f in 5 iterations, |gradient| at the start %.3g" % (v0, v1, np.abs(g0).max()))
    assert np.isfinite(v1) and v1 > v0
    with pytest.raises(ValueError):
        model.Observe(x0[:-1])
