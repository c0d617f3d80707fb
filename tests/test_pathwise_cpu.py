"""What of the pathwise samples (gogp_pathwise_*, gogp_amd/pathwise.py) can be checked without a GPU.  The first test fails
without the feature: neither the module nor the symbols exist."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from gogp_amd import _lib, kernel, pathwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gogp_pathwise_create", "gogp_pathwise_eval", "gogp_pathwise_get_v", "gogp_pathwise_destroy")


def host(simil, ndim, theta):
    """What spectral_features reads of a GP: no device needed."""
    return SimpleNamespace(NDim=ndim, Simil=simil, ThetaSimil=list(theta))


def test_symbols_declared_bound_and_mirrored():
    table = {name for name, _, _ in _lib.SYMBOLS}
    hooks = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    header = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    hpp = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    go = open(os.path.join(ROOT, "go", "gogp", "gp.go")).read()
    for name in NAMES:
        assert name in table and ("int %s(" % name) in header
    for name in ("gogp_pathwise_create", "gogp_pathwise_eval", "gogp_pathwise_destroy"):
        assert name in hpp and name in go
    assert {"gogp_test_pw_features", "gogp_test_pw_crossgrad"} <= hooks
    z = np.zeros(1)
    dp = z.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert _lib.lib().gogp_pathwise_eval(None, dp, 1, dp, None) == _lib.GOGP_EARG


def test_ard_normal_frequencies_are_the_normals_over_the_lengths():
    g = np.random.default_rng(1).standard_normal((7, 3))
    lengths = [0.5, 2.0, 1.25]
    Omega, phase, amp = pathwise.spectral_features(host(kernel.ARD(kernel.Normal, 3), 3, lengths), 7, normals=g,
                                                   rng=np.random.default_rng(2))
    assert np.array_equal(Omega, g / np.array(lengths))
    assert np.array_equal(amp, np.full(7, np.sqrt(2.0 / 7))) and np.all((phase >= 0) & (phase < 2 * np.pi))


@pytest.mark.parametrize("simil, theta", [
    (kernel.Normal, [0.8]),
    (kernel.Scaled(kernel.Matern32), [1.7, 0.6]),
    (kernel.Sum([kernel.Scaled(kernel.Normal), kernel.Scaled(kernel.Matern52Textbook)]), [0.5, 0.9, 1.5, 0.4]),
], ids=["normal", "matern32", "sum"])
def test_features_reproduce_the_kernel(simil, theta):
    """phi(x)^T phi(x') is a sum of R independent summands (2 c / R) cos(a) cos(b), each bounded by 2 c / R; with the
    uniform phase E[cos^2 cos^2] <= 3/8, so the sum's standard deviation is below c sqrt(1.5 / R) < c sqrt(2 / R): the
    bound is five of those, derived, not measured."""
    R, D = 1 << 16, 2
    rng = np.random.default_rng(7)
    gp = host(simil, D, theta)
    Omega, phase, amp = pathwise.spectral_features(gp, R, rng=rng)
    c = sum(theta[t.scale_idx] if t.scale_idx >= 0 else 1.0 for t in simil.terms)
    xa, xb = rng.uniform(-1, 1, (10, D)), rng.uniform(-1, 1, (10, D))
    for a, b in zip(xa, xb):
        got = (amp * np.cos(Omega @ a + phase)) @ (amp * np.cos(Omega @ b + phase))
        want = simil.Observe(list(theta) + list(a) + list(b))
        assert abs(got - want) <= 5 * c * np.sqrt(2.0 / R), (got, want)


@pytest.mark.parametrize("simil, theta", [(kernel.Periodic, [1.0, 2.0]), (kernel.Scaled(kernel.Matern52), [1.0, 1.0])])
def test_kernels_without_a_spectral_measure_are_refused(simil, theta):
    with pytest.raises(ValueError, match="Periodic|not a Matern"):
        pathwise.spectral_features(host(simil, 1, theta), 16)
