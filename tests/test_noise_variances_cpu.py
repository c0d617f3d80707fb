"""Per-observation noise variances without a GPU: the dense reference of tests/noise_variances_ref.py against central
differences of its own LML (dv and the [theta | phi] chain rule of HeteroscedasticModel), the conditioning of every case
the GPU tests use, gogp_noise_variances_check (host only) and the five symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import noise_variances_ref as NV
from gogp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Central differences of the reference LML at n = 40, step H: O(H^2) truncation plus eps / H rounding of an LML of size
# ~10, so no bound is fixed in advance.  Measured on the inputs below (printed by the tests), relative to the largest
# component: dv 5.2e-9 (step H s2 = 1e-7 on components of size ~50), theta 3.5e-11, [theta | phi] 2.0e-11.  The bounds are
# 10 x that.
H = 1e-5
FD_DV_BOUND = 5.2e-8
FD_THETA_BOUND = 3.5e-10
FD_HETERO_BOUND = 2.0e-10


def _ref40(fam=NV.MAIN):
    D, simil, _ = NV.FAMILIES[fam]
    X, y, v, _ = NV.inputs(40, D)
    return NV.Ref(D, simil, X, y, v), v


def _central(f, x0, h):
    g = np.zeros(len(x0))
    for i in range(len(x0)):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2.0 * h)
    return g


def test_dv_against_central_differences():
    r, v = _ref40()
    x = NV.log_theta(NV.MAIN)
    r.observe(x)
    assert (v == 0.0).sum() >= 3 and (v > 0.0).sum() >= 3
    # (a step below v_i = 0 is fine for the reference: K stays positive definite through s2)
    fd = _central(lambda vv: r.lml_only(x, vv), v, H * NV.S2)
    rel = np.abs(fd - r.dv).max() / np.abs(r.dv).max()
    print("dv against central differences: %.3e of the largest component" % rel)
    assert rel <= FD_DV_BOUND
    # ... and the theta part of the same reference, which the GPU's gradient is held to
    fdt = _central(lambda xx: r.lml_only(xx), x, H)
    relt = np.abs(fdt - r.grad).max() / np.abs(r.grad).max()
    print("theta gradient against central differences: %.3e" % relt)
    assert relt <= FD_THETA_BOUND


def test_hetero_chain_rule_against_central_differences():
    r, _ = _ref40()
    n = 40
    G = np.zeros((n, 3))  # two one-hot instruments and a drift
    G[: n // 2, 0] = 1.0
    G[n // 2:, 1] = 1.0
    G[:, 2] = np.linspace(-1.0, 1.0, n)
    x = np.concatenate([NV.log_theta(NV.MAIN), np.log([0.5 * NV.S2, 2.0 * NV.S2]), [0.3]])
    _, g = r.hetero(x, G)
    fd = _central(lambda xx: r.hetero(xx, G)[0], x, H)
    rel = np.abs(fd - g).max() / np.abs(g).max()
    print("[theta | phi] against central differences: %.3e of the largest component" % rel)
    assert rel <= FD_HETERO_BOUND


def test_noise_component_is_the_sum_of_dv():
    """UniformNoise: dK / d log theta_n = 2 s2 I, so the gradient's noise component is 2 s2 sum_i dv_i."""
    r, _ = _ref40()
    r.observe(NV.log_theta(NV.MAIN))
    assert abs(r.grad[-1] - 2.0 * NV.S2 * r.dv.sum()) <= 1e-12 * abs(r.grad).max()


def _cond(fam, n, events=None):
    D, simil, _ = NV.FAMILIES[fam]
    X, y, v, _ = NV.inputs(n, D)
    return np.linalg.cond(NV.Ref(D, simil, X, y, v, events=events).gram(NV.log_theta(fam)))


@pytest.mark.parametrize("n", NV.SHAPES)
def test_conditioning_of_the_shapes(n):
    c = _cond(NV.MAIN, n)
    print("cond(K) at n = %d: %.3e" % (n, c))
    assert c <= NV.COND_MAX


@pytest.mark.parametrize("fam", NV.FOUR)
def test_conditioning_of_the_families(fam):
    c = _cond(fam, 300)
    print("cond(K) of %s at n = 300: %.3e" % (fam, c))
    assert c <= NV.COND_MAX
    if fam == "matern52":
        assert _cond(fam, 300, events=NV.EVENTS) <= NV.COND_MAX


def test_variances_have_exact_zeros_and_the_stated_range():
    for n in NV.SHAPES[2:]:
        v = NV.variances(n)
        assert (v == 0.0).sum() >= 3 and v.min() >= 0.0 and v.max() <= 4.0 * NV.S2 and np.isfinite(v).all()
        assert v.max() > 2.0 * NV.S2  # the range is used


def test_noise_variances_check():
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    good = np.array([0.0, 1e-300, 0.5, 1e300])
    assert L.gogp_noise_variances_check(dp(good), 4) == _lib.GOGP_OK
    assert L.gogp_noise_variances_check(None, 0) == _lib.GOGP_OK
    assert L.gogp_noise_variances_check(dp(good), 0) == _lib.GOGP_OK
    assert L.gogp_noise_variances_check(None, 3) == _lib.GOGP_EARG
    assert L.gogp_noise_variances_check(dp(good), -1) == _lib.GOGP_EARG
    for bad in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        for at in range(4):
            v = good.copy()
            v[at] = bad
            assert L.gogp_noise_variances_check(dp(v), 4) == _lib.GOGP_EARG, (bad, at)
    assert L.gogp_noise_variances_check(dp(np.array([-0.0])), 1) == _lib.GOGP_OK


def test_symbols_bound_and_declared():
    """Fails on the parent commit: the five calls are in the binding's table with their argument counts, in the
    library, and declared by include/gogp_hip.h; the kernels' hooks are in the hook table."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    counts = {"gogp_noise_variances_check": 2, "gogp_set_noise_variances": 3, "gogp_get_noise_variances": 2,
              "gogp_noise_variances_gradient": 2, "gogp_append_noisy": 5}
    with open(os.path.join(ROOT, "include", "gogp_hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name, k in counts.items():
        assert name in table and len(table[name][1]) == k
        m = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == k, name
        assert getattr(L, name)
    hooks = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    assert {"gogp_test_" + k for k in _lib.NOISEVAR_HOOKS} <= hooks and "gogp_test_nv_append_commit" in hooks
    H_ = _lib.hooks()
    for name in ("gogp_test_nv_diag_add", "gogp_test_nv_gradient", "gogp_test_nv_append_commit", "gogp_test_append_commit"):
        assert getattr(H_, name)


def test_host_layer_exists():
    from gogp_amd import gp
    for name in ("SetNoiseVariances", "NoiseVariancesGradient", "Absorb", "Append"):
        assert callable(getattr(gp.GP, name))
    assert isinstance(gp.GP.NoiseVariances, property)
    assert callable(gp.HeteroscedasticModel) and callable(gp.noise_variances_kernel_check)
    with pytest.raises(ValueError):
        gp.HeteroscedasticModel(None, np.zeros(4))
