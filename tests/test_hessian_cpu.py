"""What of the LML Hessian (gogp_lml_hessian, gogp_amd/hessian.py, csrc/hessian.hip) can be checked without a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from gogp_amd import _lib, hessian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_mirrored():
    table = {name: args for name, _, args in _lib.SYMBOLS}
    assert len(table["gogp_lml_hessian"]) == 2
    assert "gogp_test_hess_kmm" in {name for name, _, _ in _lib.HOOK_SYMBOLS}
    header = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    assert re.search(r"int gogp_lml_hessian\(gogp_handle \*h, double \*H", header)
    assert "gogp_lml_hessian" in open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    assert "gogp_lml_hessian" in open(os.path.join(ROOT, "go", "gogp", "gp.go")).read()
    H = np.zeros(4)
    assert _lib.lib().gogp_lml_hessian(None, H.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == _lib.GOGP_EARG


def test_laplace_from_hessian_closed_form():
    H = np.array([[-4.0, 1.0], [1.0, -3.0]])
    r = hessian.laplace_from_hessian(-12.5, H)
    det = 4.0 * 3.0 - 1.0
    np.testing.assert_allclose(r["cov"], np.array([[3.0, 1.0], [1.0, 4.0]]) / det, rtol=1e-14)
    np.testing.assert_allclose(r["stderr"], np.sqrt([3.0 / det, 4.0 / det]), rtol=1e-14)
    assert abs(r["evidence"] - (-12.5 + np.log(2 * np.pi) - 0.5 * np.log(det))) < 1e-13
    # a log prior's Hessian is added before anything else
    r2 = hessian.laplace_from_hessian(-12.5, H + np.eye(2), log_prior=-np.eye(2))
    np.testing.assert_allclose(r2["cov"], r["cov"], rtol=1e-14)
    with pytest.raises(ValueError):
        hessian.laplace_from_hessian(0.0, np.array([[-1.0, 2.0], [2.0, -1.0]]))


def test_new_kernels_are_in_the_library_and_inside_the_limits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_audit
    ks = [k for k in codeobj_audit.kernels(_lib.LIB_PATH) if "hess_" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for want in ("hess_kmm_kernel", "hess_pair_kernel", "hess_kvec_kernel", "hess_trdot_kernel", "hess_sum_kernel"):
        assert want in names
    assert codeobj_audit.violations(ks) == []
