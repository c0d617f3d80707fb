"""gogp_amd.pathwise.draw / Paths on the GPU (run with -m gpu) against the long-double evaluation of Matheron's rule
    f_s(z) = phi(z)^T w_s + k(z, X) v_s,   v_s = K^^-1 (y - Phi(X) w_s - sqrt(sigma^2 + v) o xi_s)
with K^ factored in long doubles (hessian_ref.inverse).  N = 37 (a ragged tile), 129 (one row past a tile), 300; the noise
standard deviation is 0.1 and the inputs lie in [0, 8)^D, several length scales wide, which keeps the condition number
of K^ below 2000 and the bound 64 N eps cond max|f| below 1e-8 max|f| (asserted).  One case carries per-observation
variances, one reaches its size by Append."""
import numpy as np
import pytest

import pathwise_ref as PR
from gogp_amd import kernel, pathwise
from gogp_amd.gp import GP, GogpError
from hessian_ref import inverse

pytestmark = pytest.mark.gpu
LD, EPS = PR.LD, PR.EPS
S, R = 3, 40

#: name -> (NDim, similarity, ThetaSimil); the noise is UniformNoise at 0.1
CASES = {
    "scaled_normal": (2, kernel.Scaled(kernel.Normal), [1.2, 0.7]),
    "ard_matern32": (3, kernel.ARD(kernel.Matern32, 3), [0.6, 0.9, 1.2]),
    "sum": (2, kernel.Sum([kernel.Scaled(kernel.Normal), kernel.Scaled(kernel.Matern52Textbook)]), [0.5, 0.6, 0.5, 0.8]),
}
WITH_VARIANCES, WITH_APPEND = ("scaled_normal", 129), ("ard_matern32", 300)


def fitted(name, n):
    """(gp, X, y, v) observed at the case's parameters."""
    D, simil, theta = CASES[name]
    rng = np.random.default_rng(n)
    X = rng.uniform(0, 8, (n, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    v = rng.uniform(0.0, 0.05, n) if (name, n) == WITH_VARIANCES else np.zeros(n)
    n0 = 200 if (name, n) == WITH_APPEND else n
    g = GP(D, simil, kernel.UniformNoise, X=X[:n0], Y=y[:n0], device=0)
    if v.any():
        g.SetNoiseVariances(v)
    g.Observe(np.log(theta + [0.1]))
    if n0 < n:
        g.Append(X[n0:], y[n0:])
    return g, X, y, v


def reference(g, X, y, v, feat, W, Xi):
    """(K^, rhs (n, S), V (n, S), f: Z -> (S, m), df: Z -> (S, m, NDim)) in long doubles."""
    terms = PR.terms_of(g)
    d = LD(0.1) ** 2 + v.astype(LD)
    K = PR.kern(terms, X, X) + np.diag(d)
    rhs = y.astype(LD)[:, None] - PR.feats(*feat, X) @ W.astype(LD) - np.sqrt(d)[:, None] * Xi.T.astype(LD)
    V = inverse(K) @ rhs
    f = lambda Z: (PR.feats(*feat, Z) @ W.astype(LD) + PR.kern(terms, Z, X) @ V).T
    df = lambda Z: (np.einsum("ird,rs->sid", PR.feats(*feat, Z, deriv=True), W.astype(LD)) +
                    np.einsum("ijd,js->sid", PR.kern(terms, Z, X, deriv=True), V))
    return K, rhs, V, f, df


@pytest.mark.parametrize("n", [37, 129, 300])
@pytest.mark.parametrize("name", list(CASES))
def test_draws_against_long_doubles(name, n):
    g, X, y, v = fitted(name, n)
    rng = np.random.default_rng(11)
    feat = pathwise.spectral_features(g, R, rng=rng)
    W, Xi = rng.standard_normal((R, S)), rng.standard_normal((S, n))
    Zall = rng.uniform(-0.5, 8.5, (65, g.NDim))
    # (after Append the process has no gradient to ask for: Gradient wants an Observe)
    grad = (lambda: b"") if (name, n) == WITH_APPEND else (lambda: g.Gradient().tobytes())
    state = lambda: (g.LML(), grad(), [a.tobytes() for a in g.Produce(Zall)])
    before = state()
    with pathwise.draw(g, S, features=feat, W=W, Xi=Xi) as paths, pathwise.draw(g, S, features=feat, W=W, Xi=Xi) as again:
        assert state() == before  # the handle is left as found
        K, rhs, Vref, f, df = reference(g, X, y, v, feat, W, Xi)
        V = paths.V
        assert again.V.tobytes() == V.tobytes() and again(Zall).tobytes() == paths(Zall).tobytes()
        Kinf = float(np.abs(K).sum(1).max())
        for s in range(S):
            res = float(np.abs(K @ V[s].astype(LD) - rhs[:, s]).max())
            assert res <= 16 * n * EPS * Kinf * np.abs(V[s]).max(), (s, res)
        ev = np.linalg.eigvalsh(K.astype(float))
        cond = ev[-1] / ev[0]
        assert 64 * n * EPS * cond < 1e-8
        worst = 0.0
        for m in (1, 65):
            Z = Zall[:m]
            F, dF = paths.gradient(Z)
            assert paths(Z).tobytes() == F.tobytes()
            for got, want in ((F, f(Z)), (dF, df(Z))):
                worst = max(worst, float(np.abs(got - want).max() / (64 * n * EPS * cond * np.abs(want).max())))
        print("%s n = %d: cond %.2e, worst |error| / bound %.3e" % (name, n, cond, worst))
        assert worst <= 1.0


def test_gradient_agrees_with_differences_of_the_value():
    """Central differences of Paths(Z) at h and h / 2, Richardson-extrapolated; entrywise tolerance 10 |D(h) - extrapolated|,
    the truncation the extrapolation removed, plus 1e-9 max|dF| for the fp64 arithmetic (as tests/hessian_ref.py)."""
    g, X, y, v = fitted("sum", 129)
    D, h = g.NDim, 1e-3
    with pathwise.draw(g, S, R=R, rng=np.random.default_rng(2)) as paths:
        Z = np.random.default_rng(3).uniform(0, 8, (5, D))
        dF = paths.gradient(Z)[1]
        diff = lambda hh: np.stack([(paths(Z + hh * e) - paths(Z - hh * e)) / (2 * hh) for e in np.eye(D)], axis=-1)
        d1, d2 = diff(h), diff(h / 2)
        ext = (4 * d2 - d1) / 3
        assert np.all(np.abs(dF - ext) <= 10 * np.abs(d1 - ext) + 1e-9 * np.abs(dF).max())


def test_paths_keep_their_bits_when_the_process_moves_on():
    g, X, y, v = fitted("scaled_normal", 37)
    Z = np.random.default_rng(4).uniform(0, 8, (65, g.NDim))
    paths = pathwise.draw(g, S, R=R, rng=np.random.default_rng(5))
    F, dF = paths.gradient(Z)
    g.Observe(np.log([0.5, 1.5, 0.3]))
    g.close()
    F2, dF2 = paths.gradient(Z)
    assert F2.tobytes() == F.tobytes() and dF2.tobytes() == dF.tobytes()
    paths.close()


def test_refusals():
    D, simil, theta = CASES["scaled_normal"]
    X = np.random.default_rng(0).uniform(0, 3, (37, D))
    y = np.sin(X.sum(1))
    x = np.log(theta + [0.1])
    draw = lambda gp, s=S, r=R: pathwise.draw(gp, s, features=(np.ones((r, D)), np.zeros(r), np.ones(r)))
    g = GP(D, simil, kernel.UniformNoise, X=X, Y=y, device=0)
    with pytest.raises(GogpError, match="nothing absorbed"):
        g._push_data()
        draw(g)
    g.Observe(x)
    for s, r, what in ((65, R, "1 <= S"), (S, 0, "1 <= R")):
        with pytest.raises(GogpError, match=what):
            draw(g, s, r)
    g.set_option("gradient_precision", 32)
    g.Observe(x)
    with pytest.raises(GogpError, match="gradient_precision"):
        draw(g)
    ev = GP(1, kernel.Events(kernel.Scaled(kernel.Normal), [(1.0, 2.0, 0.5)]), kernel.UniformNoise, X=X[:, :1], Y=y, device=0)
    ev.Observe(x)
    with pytest.raises(GogpError, match="event discounts"):
        pathwise.draw(ev, S, features=(np.ones((R, 1)), np.zeros(R), np.ones(R)))
