"""The numpy reference of the explicit basis functions (tests/basis_ref.py) pinned to three independent restatements of
Rasmussen & Williams section 2.7, its gradient to central differences, and the cap that keeps the GPU tolerances of
tests/test_basis_gpu.py honest: cond(H^T K^-1 H) <= 1e6 for every case that file runs, so that beta carries at most
~1e6 * 2.2e-16 = 2e-10 relative error in the reference -- far inside rtol = 1e-6.  Also the host-side builders of
gogp_amd.basis.  No GPU.

Restatements:
  * the restricted likelihood of the projected data, lml_b = log N(N^T y; 0, N^T K N) - 1/2 log|H^T H| with N an
    orthonormal basis of null(H^T) (scipy.linalg.null_space): 1e-10 relative;
  * the universal-kriging system [[K, H], [H^T, 0]] for mu_b and sigma_b^2: 1e-10;
  * a proper prior beta ~ N(0, s2 I) (R&W eq. 2.41 - 2.43): lml_s + p/2 log s2 -> lml_b, mu_s -> mu_b, the difference
    falling as 1 / s2 over s2 = 1e4, 1e6, 1e8.  Eq. 2.43 is evaluated through A_s = I / s2 + H^T K^-1 H (the form the book
    gives; K + s2 H H^T itself has a condition number ~ s2 n / noise and loses the digits that show the 1 / s2); at
    s2 = 1e4 it is also compared with log N(y; 0, K + s2 H H^T) formed directly.
"""
import numpy as np
import pytest
import scipy.linalg

import basis_ref as BR
import loo_ref as LR
from gogp_amd import basis

N, P = 40, 3


def _small(fam="matern52", n=N, p=P, events=False):
    return BR.case(fam, n, p, events)


def _lognormal(y, K):
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, y)
    return -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * len(y) * BR.LOG_2PI


@pytest.mark.parametrize("fam,n,p", [("matern52", 40, 3), ("ard_rbf3", 60, 5), ("ard_rbf3", 90, 33)])
def test_restricted_likelihood(fam, n, p):
    r = BR.case(fam, n, p)
    Nn = scipy.linalg.null_space(r["H"].T)
    assert Nn.shape == (n, n - p)
    want = _lognormal(Nn.T @ r["y"], Nn.T @ r["K"] @ Nn) - 0.5 * np.linalg.slogdet(r["H"].T @ r["H"])[1]
    print("%s n = %d p = %d: lml_b %.15e, restricted %.15e" % (fam, n, p, r["lml"], want))
    assert abs(r["lml"] - want) <= 1e-10 * abs(want)


@pytest.mark.parametrize("fam,n,p,events", [("matern52", 40, 3, False), ("matern52", 40, 3, True), ("ard_rbf3", 60, 5, False)])
def test_universal_kriging(fam, n, p, events):
    r = BR.case(fam, n, p, events)
    D, simil, _ = BR.FAMILIES[fam]
    Ks, prior = BR.cross(D, simil, r["lt"], r["X"], r["Z"], BR.EVENTS if events else None)
    S = np.block([[r["K"], r["H"]], [r["H"].T, np.zeros((p, p))]])
    rhs = np.concatenate([Ks, r["Hz"].T], axis=0)
    sol = np.linalg.solve(S, rhs)
    mu = sol[:n].T @ r["y"]
    var = prior - (rhs * sol).sum(0)
    print("universal kriging: mu max |diff| %.3e, var max |diff| %.3e"
          % (np.abs(mu - r["mu"]).max(), np.abs(var - r["sigma"] ** 2).max()))
    np.testing.assert_allclose(r["mu"], mu, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["sigma"] ** 2, var, rtol=1e-10, atol=1e-10)


def test_proper_prior_limit():
    r = _small()
    K, H, y, n, p = r["K"], r["H"], r["y"], N, P
    L = np.linalg.cholesky(K)
    solve = lambda B: np.linalg.solve(L.T, np.linalg.solve(L, B))  # noqa: E731
    alpha, W = solve(y), solve(H)
    g = H.T @ alpha
    D, simil, _ = BR.FAMILIES["matern52"]
    Ks, _ = BR.cross(D, simil, r["lt"], r["X"], r["Z"])
    Rm = r["Hz"] - Ks.T @ W
    dl, dm = [], []
    for s2 in (1e4, 1e6, 1e8):
        As = np.eye(p) / s2 + H.T @ W
        bs = np.linalg.solve(As, g)
        lml_s = (-0.5 * y @ alpha + 0.5 * g @ bs - np.log(np.diag(L)).sum() - 0.5 * p * np.log(s2)
                 - 0.5 * np.linalg.slogdet(As)[1] - 0.5 * n * BR.LOG_2PI)  # R&W eq. 2.43 with b = 0, B = s2 I
        if s2 == 1e4:
            direct = _lognormal(y, K + s2 * H @ H.T)
            assert abs(direct - lml_s) <= 1e-6 * abs(lml_s), (direct, lml_s)
        dl.append(abs(lml_s + 0.5 * p * np.log(s2) + 0.5 * p * BR.LOG_2PI - r["lml"]))
        dm.append(np.abs(Ks.T @ alpha + Rm @ bs - r["mu"]).max())
    print("proper prior: |lml_s - lml_b| = %s, max |mu_s - mu_b| = %s" % (dl, dm))
    floor_l, floor_m = 1e-12 * abs(r["lml"]), 1e-12 * np.abs(r["mu"]).max()
    for d, floor in ((dl, floor_l), (dm, floor_m)):
        assert d[0] > 0.0
        assert d[1] <= max(d[0] / 30.0, floor) and d[2] <= max(d[1] / 30.0, floor), d
        assert d[1] >= d[0] / 300.0 or d[1] <= floor, d  # roughly 1 / s2, not faster


@pytest.mark.parametrize("fam,events", [(f, False) for f in sorted(BR.FAMILIES)] + [(BR.EVENT_FAMILY, True)])
def test_gradient_central_differences(fam, events):
    D, simil, _ = BR.FAMILIES[fam]
    ev = BR.EVENTS if events else None
    r = BR.case(fam, 40, 3, events)
    x = r["lt"]
    h = 1e-5
    fd = np.zeros_like(x)
    for k in range(len(x)):
        e = np.zeros_like(x)
        e[k] = h
        up = BR.reference(D, simil, x + e, r["X"], r["y"], r["H"], ev, want_grad=False)[1]["lml"]
        dn = BR.reference(D, simil, x - e, r["X"], r["y"], r["H"], ev, want_grad=False)[1]["lml"]
        fd[k] = (up - dn) / (2 * h)
    scale = np.abs(fd).max()
    print("%s%s: gradient max |analytic - central| = %.3e of %.3e" % (fam, " events" if events else "",
                                                                     np.abs(fd - r["grad"]).max(), scale))
    assert np.abs(fd - r["grad"]).max() <= 1e-7 * scale


def test_invariant_under_a_shift_in_the_span_of_the_basis():
    r = _small()
    c = np.array([3.0, -40.0, 7.5])
    d2 = BR.dense(r["K"], r["y"] + r["H"] @ c, r["H"])
    assert abs(d2["lml"] - r["lml"]) <= 1e-9 * abs(r["lml"])
    np.testing.assert_allclose(d2["alpha"], r["alpha"], rtol=1e-8, atol=1e-9 * np.abs(r["alpha"]).max())
    np.testing.assert_allclose(d2["beta"], r["beta"] + c, rtol=1e-9)
    np.testing.assert_array_equal(d2["cov"], r["cov"])  # sigma_b depends on y through nothing


@pytest.mark.parametrize("fam,n,p,events", BR.GPU_CASES)
def test_condition_cap_of_the_gpu_cases(fam, n, p, events):
    D, simil, _ = BR.FAMILIES[fam]
    X, _, Z = BR.inputs(n, 1, D)
    H, _ = BR.case_basis(X, Z, p)
    K = LR.gram(D, simil, BR.log_theta(fam), X, BR.EVENTS if events else None)
    W = np.linalg.solve(K, H)
    cond = np.linalg.cond(H.T @ W)
    print("%s n = %d p = %d%s: cond(A) = %.3e" % (fam, n, p, " events" if events else "", cond))
    assert n > p and cond <= 1e6


# ---- the builders -------------------------------------------------------------------------------------------------------
def test_polynomial():
    X = np.array([[0.0, 10.0], [1.0, 20.0], [4.0, 40.0]])
    H = basis.polynomial(X, 2)
    assert H.shape == (3, 5)
    np.testing.assert_array_equal(H[:, 0], 1.0)
    t0, t1 = (X[:, 0] - 2.0) / 2.0, (X[:, 1] - 25.0) / 15.0
    np.testing.assert_allclose(H[:, 1:], np.stack([t0, t0 ** 2, t1, t1 ** 2], axis=1), rtol=1e-15)
    assert np.abs(H).max() <= 1.0
    c, s = basis.polynomial_frame(X, [1])
    np.testing.assert_array_equal((c, s), ([25.0], [15.0]))
    Hz = basis.polynomial(np.array([[9.0, 55.0]]), 1, axes=[1], center=c, scale=s)
    np.testing.assert_allclose(Hz, [[1.0, 2.0]])
    np.testing.assert_array_equal(basis.polynomial(X, 0), np.ones((3, 1)))
    np.testing.assert_array_equal(basis.polynomial(np.array([5.0, 5.0]), 1), [[1.0, 0.0], [1.0, 0.0]])  # a constant coordinate
    for bad in (dict(degree=-1), dict(degree=1, axes=[2]), dict(degree=1, scale=0.0), dict(degree=1, center=np.nan)):
        with pytest.raises(ValueError):
            basis.polynomial(X, **bad)


def test_fourier():
    x = np.linspace(0.0, 3.0, 7)
    H = basis.fourier(x, 1.5, 2)
    assert H.shape == (7, 4)
    w = 2 * np.pi * x / 1.5
    np.testing.assert_allclose(H, np.stack([np.sin(w), np.cos(w), np.sin(2 * w), np.cos(2 * w)], axis=1), rtol=1e-15)
    H2 = basis.fourier(np.stack([x * 0, x], axis=1), 1.5, 1, axis=1)
    np.testing.assert_array_equal(H2, H[:, :2])
    for bad in (dict(period=0.0, harmonics=1), dict(period=1.0, harmonics=0), dict(period=1.0, harmonics=1, axis=1),
                dict(period=np.inf, harmonics=1)):
        with pytest.raises(ValueError):
            basis.fourier(x, **bad)


def test_stack_drops_a_repeated_constant():
    x = np.linspace(-1.0, 1.0, 5)
    a, b = basis.polynomial(x, 1), basis.fourier(x, 2.0, 1)
    H = basis.stack(a, b, basis.polynomial(x, 2))
    assert H.shape == (5, 2 + 2 + 2)
    np.testing.assert_array_equal(H[:, :2], a)
    np.testing.assert_array_equal(H[:, 2:4], b)
    np.testing.assert_array_equal(H[:, 4:], basis.polynomial(x, 2)[:, 1:])
    np.testing.assert_array_equal(basis.stack(np.ones(5), x), np.stack([np.ones(5), x], axis=1))
    with pytest.raises(ValueError):
        basis.stack(a, b[:4])
    with pytest.raises(ValueError):
        basis.stack()


def test_transposed_padded_layout():
    H = np.arange(12.0).reshape(4, 3) + 1.0
    Ht = basis.transposed_padded(H, 256)
    assert Ht.shape == (3, 256) and Ht.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(Ht[:, :4], H.T)
    assert not Ht[:, 4:].any()
    with pytest.raises(ValueError):
        basis.transposed_padded(H, 3)


def test_the_case_bases_are_what_the_gpu_file_assumes():
    X, _, Z = BR.inputs(300, 5, 3)
    for p in BR.COUNTS:
        H, Hz = BR.case_basis(X, Z, p)
        assert H.shape == (300, p) and Hz.shape == (5, p)
        np.testing.assert_array_equal(H[:, 0], 1.0)
        assert np.isfinite(H).all() and np.abs(H).max() <= (1.0 if p <= 5 else 6.0)
        if p > 5:
            np.testing.assert_allclose(H.T @ H, 300 * np.eye(p), atol=1e-9)


def test_basis_symbols_are_bound():
    from gogp_amd import _lib
    names = {s[0] for s in _lib.SYMBOLS}
    for f in ("set", "lml", "gradient", "get_beta", "get_alpha", "produce"):
        assert "gogp_basis_" + f in names
    hooks = {s[0] for s in _lib.HOOK_SYMBOLS}
    for k in _lib.BASIS_HOOKS:
        assert "gogp_test_" + k in hooks


# ---- the hooks of basis.hip refuse before they touch a device -------------------------------------------------------------
#: valid arguments of a small launch of every hook; an array's entry is its length, the SHORTEST the hook accepts
HOOK_VALID = {
    "basis_symm": dict(ldk=256, n=200, npad=256, ld=256, p=5, Kinv=256 * 256, Ht=5 * 256, part=None, Wt=8 * 256),
    "basis_gram": dict(ld=256, n=200, p=5, Ht=5 * 256, Wt=5 * 256, alpha=200, part=None, Ag=30),
    "basis_finish": dict(p=5, Ag=30, LA=25, Ainv=25, beta=5, scal=2, info=1),
    "basis_cols": dict(ld=256, n=200, p=5, Wt=5 * 256, LA=25, beta=5, alpha=200, Ct=8 * 256),
    "basis_predict": dict(ldkw=128, m=3, p=5, Hz=15, KW=2 * 128 + 5, beta=5, Ainv=25, mu0=3, prior=3, q=3, mu=3, sigma=3),
}


def _hook_call(hooks, which, **over):
    import ctypes
    a = dict(HOOK_VALID[which], **over)
    args, keep = [-1], []
    for name, kind in _lib_mod().BASIS_HOOKS[which]:
        if kind in "ao":
            arr = None if a[name] is None else np.zeros(max(a[name], 1))
            keep.append(arr)
            args += [None if arr is None else arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a[name] or 0]
        else:
            args.append(float(a[name]) if kind == "d" else int(a[name]))
    return getattr(hooks, "gogp_test_" + which)(*args)


def _lib_mod():
    from gogp_amd import _lib
    return _lib


def test_hooks_refuse_before_the_device_is_touched():
    """device = -1 is enough to see it: GOGP_EARG for an array one element short, a NULL array and the shapes no launch
    can take; the valid call gets as far as the device (GOGP_OK with one, GOGP_EHIP without)."""
    L = _lib_mod()
    L.build()
    hooks = L.hooks()
    EARG, OKS = L.GOGP_EARG, (L.GOGP_OK, L.GOGP_EHIP)
    assert hooks.gogp_test_basis_symm_slabs(200) == 4 and hooks.gogp_test_basis_gram_slabs(200) == 1
    assert hooks.gogp_test_basis_symm_slabs(16384) == 4 and hooks.gogp_test_basis_gram_slabs(16384) == 64
    assert hooks.gogp_test_basis_symm_slabs(0) == 0 and hooks.gogp_test_basis_gram_slabs(0) == 0
    HOOK_VALID["basis_symm"]["part"] = 4 * 8 * 256
    HOOK_VALID["basis_gram"]["part"] = 30
    for which, valid in HOOK_VALID.items():
        assert _hook_call(hooks, which) in OKS, which
        for name, kind in L.BASIS_HOOKS[which]:
            if kind in "ao":
                assert _hook_call(hooks, which, **{name: valid[name] - 1}) == EARG, (which, name, "short")
                if (which, name) == ("basis_predict", "sigma"):  # optional: NULL with length 0 skips the deviation
                    assert _hook_call(hooks, which, sigma=None) in OKS
                    continue
                assert _hook_call(hooks, which, **{name: None}) == EARG, (which, name, "NULL")
        for bad in (dict(p=0), dict(p=65)):
            assert _hook_call(hooks, which, **bad) == EARG, (which, bad)
    for bad in (dict(n=0), dict(n=257), dict(npad=128), dict(ld=255), dict(ldk=255)):
        assert _hook_call(hooks, "basis_symm", **bad) == EARG, bad
    for which in ("basis_gram", "basis_cols"):
        for bad in (dict(n=0), dict(ld=199)):
            assert _hook_call(hooks, which, **bad) == EARG, (which, bad)
    for bad in (dict(m=0), dict(ldkw=4)):
        assert _hook_call(hooks, "basis_predict", **bad) == EARG, bad
