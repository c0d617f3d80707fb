"""One handle walked through the factorisation sweep's schedules without being recreated (run with -m gpu).

Every evaluation enters through one routine that waits for what the previous one left running and resets what the
handle says about the old factor (gogp_amd/csrc/api.hip: begin_evaluation), and the sweep and the lazy inverse walk
the same super-panels through the same stages.  The walk crosses what follows from that in combination: the fused
sweep, the lazy inverse, K^-1 in two launches, the other chain form, the float inverse, the one-launch path for
N <= 128 and the single-stream order, each on the state its predecessor left behind.

N = 1700 with superpanel_head = 4, head_remaining = 3, superpanel = 2: seven panels in super-panels of 4 + 2 + 1 --
every group size of the updates inside a super-panel, two different widths of the next super-panel, a one-panel tail.

After every step the oracle's LML (rel 1e-8), gradient (1e-6 of max(1, max|g|); under gradient_precision = 32 the
1e-6 of max|g| of tests/test_schedule_regimes_gpu.py) and Alpha (rtol 1e-6, atol 1e-8); and bit for bit what the
library promises: the LML does not depend on eager, lookahead or gradient_precision, the gradient not on kinv_split, a
repeated evaluation returns itself, and the handle at the end of the walk returns what a fresh one returns.
"""
import numpy as np
import pytest

from gogp_amd import kernel

pytestmark = pytest.mark.gpu

N, N_TINY, D = 1700, 100, 3
SIMIL, NOISE = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
LOG_THETA = np.log([0.9, 0.5, 0.15])   # as test_lazy_and_eager_paths_agree_bitwise_on_lml: comfortably positive definite
SUPERPANELS = (("superpanel_head", 4), ("head_remaining", 3), ("superpanel", 2))


def _inputs():
    rng = np.random.default_rng(43)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=N)
    return X, (y - y.mean()) / y.std()


@pytest.fixture(scope="module")
def reference():
    """The oracle's (LML, gradient, Alpha) at N = 1700 and on the first 100 rows, computed once."""
    from oracle.oracle import FastOracle
    X, y = _inputs()
    out = {}
    for n in (N, N_TINY):
        o = FastOracle(D, SIMIL, NOISE)
        o.set_data(X[:n], y[:n])
        out[n] = (o.Observe(LOG_THETA), o.Gradient(), o.Alpha.copy())
    return out


def _new_handle(options=()):
    from gogp_amd.gp import GP
    X, y = _inputs()
    g = GP(D, SIMIL, NOISE, X=X, Y=y)
    for name, value in SUPERPANELS + tuple(options):
        g.set_option(name, value)
    return g


def _evaluate(g, ref, step, mixed=False):
    """Observe + Gradient + Alpha of the handle, held against the oracle's."""
    lml_o, grad_o, alpha_o = ref
    lml, grad, alpha = g.Observe(LOG_THETA), g.Gradient(), g.Alpha
    gmax = np.abs(grad_o).max()
    print("SWEEP %-28s lml rel %.2e  grad %.2e of max|g| = %.3g  alpha %.2e" % (
        step, abs(lml - lml_o) / abs(lml_o), np.abs(grad - grad_o).max() / gmax, gmax,
        np.abs(alpha - alpha_o).max()), flush=True)
    assert abs(lml - lml_o) <= 1e-8 * abs(lml_o), (step, lml, lml_o)
    assert np.abs(grad - grad_o).max() <= 1e-6 * (gmax if mixed else max(1.0, gmax)), (step, grad, grad_o)
    np.testing.assert_allclose(alpha, alpha_o, rtol=1e-6, atol=1e-8, err_msg=step)
    return lml, grad, alpha


def test_one_handle_walked_through_the_sweeps_schedules(reference):
    X, y = _inputs()
    g = _new_handle()
    lml0, grad0, alpha0 = _evaluate(g, reference[N], "default")
    lml, grad, alpha = _evaluate(g, reference[N], "default again")
    assert lml == lml0
    np.testing.assert_array_equal(grad, grad0)
    np.testing.assert_array_equal(alpha, alpha0)

    g.set_option("eager", 0)   # the triangular inverse on demand, alpha by backward substitution
    assert _evaluate(g, reference[N], "eager = 0")[0] == lml0
    g.set_option("eager", 1)

    g.set_option("kinv_fused", 0)   # K^-1 = Y Y^T in two launches, the first inside the sweep; then in one
    g.set_option("kinv_split", 60)
    _, grad_split, _ = _evaluate(g, reference[N], "kinv_fused = 0, kinv_split = 60")
    g.Observe(LOG_THETA)   # ... and an early launch that no Gradient picks up, left for the next evaluation's entry
    g.set_option("kinv_split", 0)
    np.testing.assert_array_equal(_evaluate(g, reference[N], "kinv_fused = 0, kinv_split = 0")[1], grad_split)
    g.set_option("kinv_split", 60)
    g.set_option("kinv_fused", -1)

    g.set_option("chain_split", 0)   # the 256-block kernel and a panel solve on the chain
    _evaluate(g, reference[N], "chain_split = 0")
    g.set_option("chain_split", -1)

    g.set_option("gradient_precision", 32)   # the inverse and K^-1 in float buffers of their own
    assert _evaluate(g, reference[N], "gradient_precision = 32", mixed=True)[0] == lml0
    g.set_option("gradient_precision", 64)
    lml, grad, _ = _evaluate(g, reference[N], "gradient_precision = 64")
    assert lml == lml0
    np.testing.assert_array_equal(grad, grad0)

    g.X, g.Y = X[:N_TINY], y[:N_TINY]   # one launch for the whole factorisation, behind a sweep's pending inverse
    lml_t, grad_t, _ = _evaluate(g, reference[N_TINY], "N = 100")
    lml, grad, _ = _evaluate(g, reference[N_TINY], "N = 100 again")
    assert lml == lml_t
    np.testing.assert_array_equal(grad, grad_t)
    g.X, g.Y = X, y
    lml, grad, _ = _evaluate(g, reference[N], "N = 1700 again")
    assert lml == lml0
    np.testing.assert_array_equal(grad, grad0)

    g.set_option("lookahead", 0)   # everything in order on the main stream
    lml, grad, alpha = _evaluate(g, reference[N], "lookahead = 0")
    assert lml == lml0
    # nothing of the walk is left in the handle: a fresh one under the same options returns the same bits
    f = _new_handle((("lookahead", 0),))
    lml_f, grad_f, alpha_f = _evaluate(f, reference[N], "lookahead = 0, fresh handle")
    f.close()
    g.close()
    assert lml == lml_f
    np.testing.assert_array_equal(grad, grad_f)
    np.testing.assert_array_equal(alpha, alpha_f)
