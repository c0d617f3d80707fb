"""GP.BlockCV / GP.BlockCVScore / GP.BlockCVGradient (gogp_blockcv, gogp_blockcv_gradient) on the GPU against the dense
closed form of tests/blockcv_ref.py (np.linalg.inv in fp64; tests/test_blockcv_cpu.py pins that closed form to one refit
per block and to central differences).  The structure, inputs, families, noise and tolerances of tests/test_loo_gpu.py:
mu, sigma, log p and their sum rtol = 1e-6, atol = 1e-8; every component of the gradient within 1e-6 of the largest
absolute component.  The conditioning argument of that file's header carries over: the diagonal blocks of K^-1 are no
worse conditioned than K (their eigenvalues interlace those of K^-1), cond(K) <~ 3e4, so the per-block Cholesky factor,
its inverse and the sums of at most 128 terms behind w and v carry ~1e-11 relative, five orders below the bound.

Shapes (family ard_rbf3, after Absorb and after Observe): n = 1; 20 as (7, 13), the one-launch `tiny` path; 128 as one
block, the LDS factorisation's limit; 129 as (128, 1), two groups; 300 as (1, 5, 64, 128, 37, 65), blocks that fill a
group, share one and straddle the 64- and 128-column boundaries; 1100 with lengths drawn from 1 .. 128 (fixed seed):
npad = 1280, several groups per 256-panel.

Reference counterpart: none."""
import ctypes

import numpy as np
import pytest

import blockcv_ref as BR
import loo_ref as LR
from gogp_amd import _lib, kernel, optimize, synth
from test_loo_gpu import FAMILIES, RADIAL, SHAPE_FAMILY, _fit, _gp, _x
from test_loo_gpu import _ref as _loo_ref

pytestmark = pytest.mark.gpu


def _random_lengths(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < n:
        out.append(min(int(rng.integers(1, 129)), n - sum(out)))
    return tuple(out)


#: n -> block lengths
SHAPES = {1: (1,), 20: (7, 13), 128: (128,), 129: (128, 1), 300: (1, 5, 64, 128, 37, 65), 1100: _random_lengths(1100)}
_REF = {}


def _fifties(n):
    from gogp_amd.gp import blocks
    return blocks(n, 50)


def _ref(fam, n, start, events=None):
    """Inputs and reference of one case: computed once, shared, read only."""
    key = (fam, n, tuple(int(s) for s in start), bool(events))
    if key not in _REF:
        D, simil, _ = FAMILIES[fam]
        X, y, _ = LR.inputs(n, 1, D)
        _REF[key] = (X, y) + BR.reference(D, simil, _x(fam), X, y, start, events)
    return _REF[key]


def _check(g, start, want, tag, gradient=True):
    """Values, score and gradient against the reference, every figure printed first; a second call: the same bits"""
    mu_o, sigma_o, logp_o, grad_o = want
    mu, sigma, logp = g.BlockCV(start)
    score = g.BlockCVScore(start)
    grad = g.BlockCVGradient(start) if gradient else None
    crit = lambda a, b: (np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))).max() if len(b) else 0.0  # noqa: E731
    print("%s: mu %.3e sigma %.3e logp %.3e of the rtol 1e-6 + atol 1e-8 criterion; score %.12e (reference %.12e)"
          % (tag, crit(mu, mu_o), crit(sigma, sigma_o), crit(logp, logp_o), score, logp_o.sum()))
    if gradient:
        scale = np.abs(grad_o).max()
        print("%s: gradient max |err| = %.3e of largest component %.3e (%.2e relative)"
              % (tag, np.abs(grad - grad_o).max(), scale, np.abs(grad - grad_o).max() / scale))
    assert logp.shape == (len(start) - 1,)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(logp, logp_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(score, logp_o.sum(), rtol=1e-6, atol=1e-8, err_msg=str(tag))
    t = 0.0
    for v in logp:  # the host's sum of the same numbers in block order
        t += v
    assert score == t
    for a, b in zip(g.BlockCV(start), (mu, sigma, logp)):
        np.testing.assert_array_equal(a, b)
    assert g.BlockCVScore(start) == score
    if gradient:
        assert grad.shape == grad_o.shape
        assert np.abs(grad - grad_o).max() <= 1e-6 * scale, (tag, grad, grad_o)
        np.testing.assert_array_equal(g.BlockCVGradient(start), grad)
    return grad


@pytest.mark.parametrize("state", ["absorb", "observe"])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_shapes(n, state):
    start = BR.starts(SHAPES[n])
    assert start[-1] == n
    X, y, *want = _ref(SHAPE_FAMILY, n, start)
    g = _gp(SHAPE_FAMILY)
    _fit(g, SHAPE_FAMILY, X, y, state)
    _check(g, start, want, (n, state))
    g.close()


def test_blocks_of_one_row_are_loo():
    n = 300
    X, y, *loo_want = _loo_ref(SHAPE_FAMILY, n)
    start = np.arange(n + 1)
    g = _gp(SHAPE_FAMILY)
    _fit(g, SHAPE_FAMILY, X, y, "observe")
    loo = g.LOO() + (g.LOOGradient(),)
    bcv = g.BlockCV(start) + (g.BlockCVGradient(start),)
    for what, a, b in zip(("mu", "sigma", "logp", "gradient"), bcv, loo):
        print("blocks of one row, %s: max |BlockCV - LOO| = %.3e (largest |LOO| %.3e)"
              % (what, np.abs(a - b).max(), np.abs(b).max()))
    for a, b in zip(bcv[:3], loo[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(g.BlockCVScore(start), g.LOOScore(), rtol=1e-6, atol=1e-8)
    assert np.abs(bcv[3] - loo[3]).max() <= 1e-6 * np.abs(loo[3]).max()
    _check(g, start, loo_want, "blocks of one row against the LOO reference")
    g.close()


@pytest.mark.parametrize("fam", sorted(RADIAL) + ["ard_rbf3", "ard_rbf64", "hyperpriors"])
def test_kernel_families(fam):
    start = _fifties(300)
    X, y, *want = _ref(fam, 300, start)
    g = _gp(fam)
    _fit(g, fam, X, y, "observe")
    _check(g, start, want, fam)
    g.close()


def test_events():
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    start = _fifties(300)
    X, y, *want = _ref(fam, 300, start, LR.EVENTS)
    plain = _ref(fam, 300, start)
    assert np.abs(want[2] - plain[4]).max() > 1e-3  # the discounts change log p ...
    assert np.abs(want[3] - plain[5]).max() > 1e-3 * np.abs(plain[5]).max()  # ... and the gradient
    g = _gp(fam, simil=kernel.Events(simil, LR.EVENTS, 0))
    _fit(g, fam, X, y, "observe")
    _check(g, start, want, "events")
    g.close()


@pytest.mark.parametrize("n", [100, 300])
def test_state_is_preserved(n):
    """Gradient, Produce, the factor, LOO and a later Append return the bits they return without the calls between"""
    fam = SHAPE_FAMILY
    D = FAMILIES[fam][0]
    X, y, *_ = _loo_ref(fam, n)
    Z = LR.inputs(1, 33, D)[2]
    X2, y2, _ = LR.inputs(5, 1, D, seed=11)
    from gogp_amd.gp import blocks
    start = blocks(n, 37)

    def run(bcv):
        g = _gp(fam)
        _fit(g, fam, X, y, "observe")
        if bcv == "first":  # the new calls form K^-1, the gradient finds it
            g.BlockCVGradient(start)
            g.BlockCV(start)
        first = (g.Gradient(), *g.Produce(Z), *g.LOO(), g.LOOGradient())
        if bcv == "between":
            g.BlockCV(start)
            g.BlockCVGradient(start)
        out = first + (g.Gradient(), *g.Produce(Z), *g.LOO(), g.LOOGradient(), g.L)
        if bcv:
            g.BlockCVGradient(start)
        g.Append(X2, y2)
        out += (g.L, g.Alpha, *g.Produce(Z))
        g.close()
        return out

    a = run(None)
    for b in (run("between"), run("first")):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
        for k in range(7):  # before and after, on the same handle
            np.testing.assert_array_equal(b[k], b[7 + k])


def test_after_append_remove_and_restore():
    from gogp_amd.gp import GogpError, blocks
    fam = SHAPE_FAMILY
    D, simil, _ = FAMILIES[fam]
    X, y, *_ = _loo_ref(fam, 300)
    X2, y2, _ = LR.inputs(5, 1, D, seed=11)
    g = _gp(fam)
    _fit(g, fam, X, y, "observe")
    old = blocks(300, 50)
    g.BlockCVGradient(old)  # the workspaces exist before the data grow
    g.Append(X2, y2)
    for call in (g.BlockCV, g.BlockCVScore, g.BlockCVGradient):  # a stale start: its last entry is not n
        with pytest.raises(GogpError) as e:
            call(old)
        assert e.value.code == _lib.GOGP_EARG
    Xa, ya = np.concatenate([X, X2]), np.concatenate([y, y2])
    start = blocks(305, 50)
    _check(g, start, BR.reference(D, simil, _x(fam), Xa, ya, start), "append 5")
    g.Remove([0, 7])
    keep = np.ones(len(ya), dtype=bool)
    keep[[0, 7]] = False
    start = blocks(303, 50)
    want = BR.reference(D, simil, _x(fam), Xa[keep], ya[keep], start)
    _check(g, start, want, "remove [0, 7]")
    L, alpha = g.L, g.Alpha
    r = _gp(fam)  # set_factor on a fresh handle
    r.X, r.Y = Xa[keep], ya[keep]
    r.restore(L, alpha)
    _check(r, start, want, "restore")
    r.close()
    g.close()


def test_contract():
    from gogp_amd.gp import GP, GogpError
    fam = SHAPE_FAMILY
    D, simil, ts = FAMILIES[fam]
    start = _fifties(300)
    X, y, *want = _ref(fam, 300, start)
    P, F = len(ts) + 1, len(start) - 1
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    g = _gp(fam)
    g.X, g.Y = X, y
    g._push_data()
    grad, total = np.zeros(P), ctypes.c_double(-1.0)
    assert L.gogp_blockcv(g._h, ip(start), F, None, None, None, ctypes.byref(total)) == _lib.GOGP_ESTATE  # nothing factored
    assert L.gogp_blockcv_gradient(g._h, ip(start), F, dp(grad), P) == _lib.GOGP_ESTATE
    g.Absorb(X, y)
    assert L.gogp_blockcv_gradient(g._h, ip(start), F, dp(grad), P + 1) == _lib.GOGP_EARG
    assert L.gogp_blockcv_gradient(g._h, ip(start), F, dp(grad), P - 1) == _lib.GOGP_EARG
    assert L.gogp_blockcv_gradient(g._h, ip(start), F, None, P) == _lib.GOGP_EARG
    # what gogp_blockcv_check refuses
    bad = {"start[0] != 0": [1, 50, 300], "an empty block": [0, 50, 50, 300], "decreasing": [0, 100, 50, 300],
           "start[F] != n": [0, 100, 200, 299], "beyond n": [0, 100, 200, 301], "a block of 129": [0, 100, 229, 300]}
    for why, st in bad.items():
        st = np.array(st, dtype=np.int64)
        assert L.gogp_blockcv(g._h, ip(st), len(st) - 1, None, None, None, ctypes.byref(total)) == _lib.GOGP_EARG, why
        assert L.gogp_blockcv_gradient(g._h, ip(st), len(st) - 1, dp(grad), P) == _lib.GOGP_EARG, why
    assert L.gogp_blockcv(g._h, None, F, None, None, None, None) == _lib.GOGP_EARG
    assert L.gogp_blockcv(g._h, ip(start), -1, None, None, None, None) == _lib.GOGP_EARG
    # NULL arrays: any subset
    logp = np.zeros(F)
    assert L.gogp_blockcv(g._h, ip(start), F, None, None, None, None) == _lib.GOGP_OK
    assert L.gogp_blockcv(g._h, ip(start), F, None, None, dp(logp), ctypes.byref(total)) == _lib.GOGP_OK
    np.testing.assert_allclose(logp, want[2], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(total.value, want[2].sum(), rtol=1e-6, atol=1e-8)
    sigma, mu = np.zeros(300), np.zeros(300)
    assert L.gogp_blockcv(g._h, ip(start), F, None, dp(sigma), None, None) == _lib.GOGP_OK
    np.testing.assert_allclose(sigma, want[1], rtol=1e-6, atol=1e-8)
    assert L.gogp_blockcv(g._h, ip(start), F, dp(mu), None, dp(logp), None) == _lib.GOGP_OK
    np.testing.assert_allclose(mu, want[0], rtol=1e-6, atol=1e-8)
    # gradient_precision = 32: K^-1 is float
    g.set_option("gradient_precision", 32)
    g.Observe(_x(fam))
    for call in (g.BlockCV, g.BlockCVScore, g.BlockCVGradient):
        with pytest.raises(GogpError) as e:
            call(start)
        assert e.value.code == _lib.GOGP_EARG
    g.close()
    g32 = GP(D, simil, LR.NOISE, ThetaSimil=ts, ThetaNoise=LR.TN, device=0, precision=32)
    g32.Absorb(X, y)
    for call in (g32.BlockCV, g32.BlockCVScore, g32.BlockCVGradient):
        with pytest.raises(GogpError) as e:
            call(start)
        assert e.value.code == _lib.GOGP_EARG
    g32.close()


def test_empty_process():
    from gogp_amd.gp import GogpError, blocks
    fam = SHAPE_FAMILY
    D, _, ts = FAMILIES[fam]
    g = _gp(fam)
    g.Absorb(np.zeros((0, D)), np.zeros(0))
    start = blocks(0, 10)
    assert list(start) == [0]
    mu, sigma, logp = g.BlockCV(start)
    assert mu.shape == sigma.shape == logp.shape == (0,)
    assert g.BlockCVScore(start) == 0.0
    grad = g.BlockCVGradient(start)
    assert grad.shape == (len(ts) + 1,) and not grad.any()
    g.Observe(_x(fam))
    assert g.BlockCVScore(start) == 0.0 and not g.BlockCVGradient(start).any()
    with pytest.raises(GogpError) as e:  # rows that do not exist
        g.BlockCVScore([0, 3])
    assert e.value.code == _lib.GOGP_EARG
    g.close()


def test_optimiser_on_the_block_objective():
    from gogp_amd.gp import GP, BlockCVModel, blocks
    n, D, threshold = 200, 2, 1e-3
    X, y = synth.make_inputs(n, D, 5)
    simil = kernel.Scaled(kernel.Normal)
    g = GP(D, simil, LR.NOISE, X=X, Y=y, device=0)
    start = blocks(n, 20)
    m = BlockCVModel(g, start)
    x0 = np.log(synth.theta0(D) * np.array([1.0, 1.0, 3.0]))
    first = m.Observe(x0)
    res = optimize.lbfgs(m, x0, gradient_threshold=threshold)
    want = BR.reference(D, simil, res.x, X, y, start)
    print("block objective: start %.9f, end %.9f (reference %.9f) after %d iterations, %d evaluations; theta = %s, "
          "max |gradient| = %.3e (reference %.3e)"
          % (first, res.lml, want[2].sum(), res.iterations, res.evaluations, np.exp(res.x), np.abs(res.grad).max(),
             np.abs(want[3]).max()))
    assert res.lml >= first
    assert res.converged and np.abs(res.grad).max() <= threshold
    np.testing.assert_allclose(res.lml, want[2].sum(), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.Observe(res.x), res.lml, rtol=1e-12, atol=0)  # the model ends at the returned point
    g.close()


def test_block_model_adds_the_priors():
    from gogp_amd.gp import GP, BlockCVModel, blocks
    fam = "matern52"
    D, simil, ts = FAMILIES[fam]
    start = blocks(129, 20)
    X, y, *want = _ref(fam, 129, start)
    pri = optimize.NormalLogPriors(np.zeros(len(ts) + 1), np.ones(len(ts) + 1))
    g = GP(D, simil, LR.NOISE, X=X, Y=y, device=0)
    x = _x(fam)
    v = BlockCVModel(g, start, pri).Observe(x)
    m = BlockCVModel(g, start, pri)
    assert m.Observe(x) == v
    np.testing.assert_allclose(v, want[2].sum() + pri.Observe(x), rtol=1e-6, atol=1e-8)
    gr = m.Gradient()
    want_g = want[3] + np.asarray(pri.Gradient())
    assert np.abs(gr - want_g).max() <= 1e-6 * np.abs(want_g).max()
    g.close()
