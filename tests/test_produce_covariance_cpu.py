"""GP.ProduceCovariance / GP.Sample without a GPU: the numpy reference of tests/produce_cov_ref.py against the marginal
reference of tests/produce_grad_ref.py and against the conditional of the explicitly built joint Gaussian, the two C ABI
symbols and their ctypes prototypes, the new kernels in the compiled code object, the slab policy's two pinned values
as the header states them, and the argument checks that precede every device call.

Reference counterpart: none (gp.GP.Produce keeps the diagonal of Kstar^T K^-1 Kstar only, gp/gp.go:341-342, 356)."""
import os
import sys

import numpy as np
import pytest

import produce_cov_ref as PC
import produce_grad_ref as PG
from gogp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj_audit  # noqa: E402


@pytest.mark.parametrize("fam", PG.FOUR)
def test_reference_diagonal_is_the_marginal_variance(fam):
    D, simil, ts = PC.FAMILIES[fam]
    X, y, Z = PC.inputs(300, 33, D)
    mu, cov = PC.reference(D, simil, ts, X, y, Z)
    mu_o, sigma_o = PG.reference(D, simil, ts, X, y, Z)[:2]
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), sigma_o, rtol=1e-12)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-12, atol=1e-15)
    assert np.array_equal(cov.shape, (33, 33))


def _joint_conditional(D, simil, ts, X, y, Z, events=None):
    """mean and covariance of f(Z) given y from the joint Gaussian of (y, f(Z)), with np.linalg.solve on K itself"""
    K, Ks, Kzz = PC.grams(D, simil, ts, X, Z, events=events)
    n = len(X)
    J = np.block([[K, Ks], [Ks.T, Kzz]])
    Jyy, Jyz, Jzz = J[:n, :n], J[:n, n:], J[n:, n:]
    return Jyz.T @ np.linalg.solve(Jyy, y), Jzz - Jyz.T @ np.linalg.solve(Jyy, Jyz)


@pytest.mark.parametrize("fam", PG.FOUR)
def test_reference_is_the_conditional_of_the_joint_gaussian(fam):
    D, simil, ts = PC.FAMILIES[fam]
    X, y, Z = PC.inputs(129, 17, D)
    mu, cov = PC.reference(D, simil, ts, X, y, Z)
    mu_j, cov_j = _joint_conditional(D, simil, ts, X, y, Z)
    assert np.abs(cov - cov_j).max() <= 1e-9 * np.abs(cov_j).max()
    assert np.abs(mu - mu_j).max() <= 1e-9 * max(1.0, np.abs(mu_j).max())


def test_reference_with_events_is_the_conditional_of_the_joint_gaussian():
    D, simil, ts = PC.FAMILIES["matern52"]
    X, y, Z, _ = PC.event_inputs(129, 33)
    mu, cov = PC.reference(D, simil, ts, X, y, Z, events=PC.EVENTS)
    plain = PC.reference(D, simil, ts, X, y, Z)[1]
    assert np.abs(cov - plain).max() > 1e-3  # the discounts matter at these inputs
    mu_j, cov_j = _joint_conditional(D, simil, ts, X, y, Z, events=PC.EVENTS)
    assert np.abs(cov - cov_j).max() <= 1e-9 * np.abs(cov_j).max()


def test_reference_without_observations_is_the_prior():
    D, simil, ts = PC.FAMILIES["ard_rbf3"]
    Z = PC.inputs(1, 6, D)[2]
    mu, cov = PC.reference(D, simil, ts, np.zeros((0, D)), np.zeros(0), Z)
    assert not mu.any()
    np.testing.assert_array_equal(cov, PC.grams(D, simil, ts, np.zeros((0, D)), Z)[2])


def test_symbols_are_exported_and_declared():
    names = [s[0] for s in _lib.SYMBOLS]
    assert "gogp_produce_covariance" in names and "gogp_produce_samples" in names
    L = _lib.lib()  # AttributeError if the library does not export one of them
    assert len(L.gogp_produce_covariance.argtypes) == 5
    assert len(L.gogp_produce_samples.argtypes) == 8
    header = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    assert "#define GOGP_COV_MAX_M 4096" in header and _lib.GOGP_COV_MAX_M == 4096
    assert ("int gogp_produce_covariance(gogp_handle *h, const double *Z, int64_t m, double *mu, double *cov /* m x m */);"
            in header)
    assert ("int gogp_produce_samples(gogp_handle *h, const double *Z, int64_t m, const double *xi, int64_t ns, "
            "double diag_add,") in header


def test_code_object_contains_the_new_kernels():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgogp_hip.so not built")
    names = [k["name"] for k in codeobj_audit.kernels(_lib.LIB_PATH)]
    for want in ("pcov_syrk_kernel", "pcov_final_kernel", "pcov_final_kernel_ev", "pcov_add_mu_kernel"):
        assert "gogp::" + want in names, want


def test_new_kernels_pass_the_audit_without_an_allow_list_entry():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgogp_hip.so not built")
    mine = [k for k in codeobj_audit.kernels(_lib.LIB_PATH) if "pcov_" in k["name"]]
    assert len(mine) >= 4
    assert not [v for v in codeobj_audit.violations(mine)]
    for table in (codeobj_audit.SGPR_SPILL_ALLOW, codeobj_audit.AGPR_ALLOW):
        assert not any("pcov" in pat for pat in table)


def test_bad_shapes_raise_before_any_device_call():
    from gogp_amd.gp import GP
    D, simil, _ = PC.FAMILIES["ard_rbf3"]
    g = GP.__new__(GP)  # no handle: a device call would fail on the missing attribute, not with ValueError
    g.NDim = D
    with pytest.raises(ValueError):
        GP.ProduceCovariance(g, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        GP.ProduceCovariance(g, np.zeros((3, 2)))  # 6 values: a reshape to (2, 3) would pass silently
    with pytest.raises(ValueError):
        GP.Sample(g, np.zeros((3, 2)))
    Z = np.zeros((4, D))
    for xi in (np.zeros((2, 5)), np.zeros((4, 2)), np.zeros(5), np.zeros((1, 2, 4))):
        with pytest.raises(ValueError):
            GP.Sample(g, Z, xi=xi)
    with pytest.raises(ValueError):
        GP.Sample(g, Z, ns=-1)
