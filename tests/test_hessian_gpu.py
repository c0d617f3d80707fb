"""gogp_lml_hessian through gogp_amd.hessian.lml_hessian on the GPU (run with -m gpu) against the long-double reference of
tests/hessian_ref.py: central differences of the analytic gradient, Richardson-extrapolated, with the tolerance that
reference derives from its own truncation.  N = 37 (a ragged tile), 129 (one row past a 128 tile), 300 (several k-steps,
a ragged last one); three descriptors: cross terms between ARD lengths (two groups of one term), a sum whose parameters of
different terms have zero mixed derivatives, with the period and a noise parameter K does not depend on, and Matern-3/2
in two dimensions.  Fails without the feature: neither the module nor the symbol exists."""
import numpy as np
import pytest

import hessian_ref as R
from gogp_amd.gp import GP
from gogp_amd.hessian import lml_hessian

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [37, 129, 300])
@pytest.mark.parametrize("name", list(R.CASES))
def test_hessian_against_reference(name, n):
    D, simil, noise, X, y, x = R.data(name, n)
    g = GP(D, simil, noise, X=X, Y=y, device=0)
    lml = g.Observe(x)
    before = (lml, g.LML(), g.Gradient().tobytes(), [a.tobytes() for a in g.LOO()[:3]])
    H = lml_hessian(g)
    Href, tol = R.hessian(name, n)
    ratio = np.abs(H - Href) / tol
    print("%s n = %d: max |H| = %.3e, largest |H - Href| / bound = %.3e at %s" %
          (name, n, np.abs(H).max(), ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape)))
    assert np.all(np.isfinite(H)) and ratio.max() <= 1.0, (H, Href, tol)
    assert np.array_equal(H, H.T)
    assert lml_hessian(g).tobytes() == H.tobytes()
    assert (lml, g.LML(), g.Gradient().tobytes(), [a.tobytes() for a in g.LOO()[:3]]) == before


# ---- against the closed forms, over the descriptor space -------------------------------------------------------------------
# hessian_ref.analytic: H_ij per parameter from K_i and K_ij in long doubles.  The allowance per entry comes from the
# reference alone: FACTOR = 8 x |analytic in float64 - analytic in long doubles|, no smaller than gamma(n) x the magnitude
# of H_ij.  FACTOR and gamma(n) are as set; the magnitude term was widened twice, each time from the reference's own numbers
# (hessian_ref.summand_magnitudes states the reasoning), and the ratios measured on an MI355X before each step are kept:
#   the sum of the magnitudes of the three terms of H_ij: 15 of 108 cases missed, by up to 6.3 x (four terms, n = 129, entry
#       (2, 8): parameters of two different terms, the difference of two traces) at |H - analytic| = 1e-13 max|H| -- the
#       traces cancel (W = alpha alpha^T - K^-1) to 1 / 70 .. 1 / 1100 of their summands;
#   the sum of the magnitudes of the terms' summands: 3 missed -- "sum" n = 1 by 1.14 x (entry (2, 2): gamma(1) is one
#       rounding for a product of several inexact factors), "sum" n = 129 by 1.53 x, "matern32" n = 37 by 1.10 x;
#   each summand times the number of its factors that come out of the factorisation (alpha, K^-1): at most 3 x the former.
# Entries that vanish identically (a ConstantNoiseParam's row and column) are exact zeros.  Worst ratios recorded on an
# MI355X: DESIGN.md section 4, the Hessian's entry.
FACTOR = 8.0


@pytest.mark.parametrize("n", [1, 37, 64, 129])
@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_hessian_against_closed_forms(name, n):
    import grad_reduce_ref as G
    D, simil, noise, X, y, x = R.data(name, n)
    g = GP(D, simil, noise, X=X, Y=y, device=0)
    v = R.variances(name, n)
    if v is not None:
        g.SetNoiseVariances(v)
    g.Observe(x)
    H = lml_hessian(g)
    A, mag = R.analytic(name, n)
    A64, _ = R.analytic(name, n, mode="f64")
    wide = np.maximum(mag, R.summand_magnitudes(name, n))
    allowed = np.maximum(FACTOR * np.abs(A64.astype(np.longdouble) - A).astype(np.float64), G.gamma(n) * wide)
    err = np.abs(H.astype(np.longdouble) - A).astype(np.float64)
    zero = mag == 0
    assert np.all(np.isfinite(H)) and not H[zero].any(), "an entry that vanishes identically is not an exact zero"
    ratio = np.divide(err, allowed, out=np.zeros_like(err), where=~zero)
    print("%s n = %d: max |H| = %.3e, largest |H - analytic| / allowed = %.3f at %s" %
          (name, n, np.abs(H).max(), ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape)))
    assert ratio.max() <= 1.0, (H, A, allowed)
    assert np.array_equal(H, H.T) and lml_hessian(g).tobytes() == H.tobytes()
    g.close()


def test_refusals():
    from gogp_amd import _lib, kernel
    from gogp_amd.gp import GogpError
    D, simil, noise, X, y, x = R.data("matern32", 37)

    def code(g):
        with pytest.raises(GogpError) as e:
            lml_hessian(g)
        return e.value.code

    g = GP(D, simil, noise, X=X, Y=y, device=0, precision=32)
    g.Observe(x)
    assert code(g) == _lib.GOGP_EARG
    g.close()
    g = GP(D, simil, noise, X=X, Y=y, device=0)
    g.set_option("gradient_precision", 32)
    g.Observe(x)
    assert code(g) == _lib.GOGP_EARG
    g.close()
    g = GP(D, kernel.Events(simil, [(-0.5, 0.25, 0.7)]), noise, X=X, Y=y, device=0)
    g.Observe(x)
    assert code(g) == _lib.GOGP_EARG
    g.close()
    g = GP(D, simil, noise, X=X, Y=y, device=0)
    assert not lml_hessian(g).any()  # no rows on the handle yet: zeros, no error
    g.SetNoiseVariances(np.zeros(len(y)))  # the one public call that puts the rows on the handle without absorbing them
    assert code(g) == _lib.GOGP_ESTATE  # rows, nothing absorbed
    g.Observe(x)
    assert np.isfinite(lml_hessian(g)).all()
    g.close()
