"""GP.ProduceGradient without a GPU: the numpy reference of tests/produce_grad_ref.py against central finite differences
of its own mu and sigma, the C ABI symbol and its ctypes prototype, the new kernels in the compiled code object, and
the argument check that precedes every device call.

Reference counterpart: none (gp.GP.Produce returns mu and sigma only)."""
import os
import sys

import numpy as np
import pytest

import produce_grad_ref as PG
from gogp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj_audit  # noqa: E402

FD_STEP = 1e-5
FD_TOL = 1e-7  # of the largest component: the central difference's own error (~ step^2 x third derivative) is ~1e-9


@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("fam", PG.FOUR)
def test_reference_agrees_with_finite_differences(fam, n):
    D, simil, ts = PG.FAMILIES[fam]
    m = 9
    X, y, Z = PG.inputs(n, m, D)
    mu, sigma, dmu, dsigma = PG.reference(D, simil, ts, X, y, Z)
    assert sigma.min() > 0.05, sigma.min()  # no s_j near zero: dsigma is well defined
    fd_mu, fd_sigma = np.zeros((m, D)), np.zeros((m, D))
    for d in range(D):
        Zp, Zm = Z.copy(), Z.copy()
        Zp[:, d] += FD_STEP
        Zm[:, d] -= FD_STEP
        mp, sp = PG.reference(D, simil, ts, X, y, Zp)[:2]
        mm, sm = PG.reference(D, simil, ts, X, y, Zm)[:2]
        fd_mu[:, d] = (mp - mm) / (2 * FD_STEP)
        fd_sigma[:, d] = (sp - sm) / (2 * FD_STEP)
    for name, got, want in (("dmu", dmu, fd_mu), ("dsigma", dsigma, fd_sigma)):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print("%s n=%d %s: %.2e of %.2e" % (fam, n, name, err, scale))
        assert err <= FD_TOL * scale, (fam, n, name, err, scale)


def test_reference_with_events_agrees_with_finite_differences():
    D, simil, ts = PG.FAMILIES["matern52"]
    X, y, Z, bounds = PG.event_inputs(129, 33)
    assert np.abs(Z - bounds[None, :]).min() >= 1e-3
    kw = dict(events=PG.EVENTS)
    _, sigma, dmu, dsigma = PG.reference(D, simil, ts, X, y, Z, **kw)
    mp, sp = PG.reference(D, simil, ts, X, y, Z + FD_STEP, **kw)[:2]
    mm, sm = PG.reference(D, simil, ts, X, y, Z - FD_STEP, **kw)[:2]
    for got, want in ((dmu, (mp - mm) / (2 * FD_STEP)), (dsigma, (sp - sm) / (2 * FD_STEP))):
        assert np.abs(got[:, 0] - want).max() <= FD_TOL * np.abs(want).max()


def test_symbol_is_exported_and_declared():
    assert "gogp_produce_gradient" in [s[0] for s in _lib.SYMBOLS]
    f = _lib.lib().gogp_produce_gradient  # AttributeError if the library does not export it
    assert len(f.argtypes) == 7
    header = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    assert "int gogp_produce_gradient(gogp_handle *h, const double *Z, int64_t m, double *mu, double *sigma," in header


def test_code_object_contains_the_new_kernels():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgogp_hip.so not built")
    names = " ".join(k["name"] for k in codeobj_audit.kernels(_lib.LIB_PATH))
    for want in ("bwd_panel_kernel<1>", "bwd_panel_kernel<2>", "bwd_panel_kernel<4>", "pgrad_kernel<4>",
                 "pgrad_kernel<8>", "pgrad_kernel<16>", "pgrad_kernel_ev<4>", "pgrad_final_kernel"):
        assert want in names, want


def test_mismatched_columns_raise_before_any_device_call():
    from gogp_amd.gp import GP
    D, simil, _ = PG.FAMILIES["ard_rbf3"]
    g = GP.__new__(GP)  # no handle: a device call would fail on the missing attribute, not with ValueError
    g.NDim = D
    with pytest.raises(ValueError):
        GP.ProduceGradient(g, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        GP.Produce(g, np.zeros((4, 2)))
