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
