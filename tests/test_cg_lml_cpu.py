"""The iterative exact GP's LML and gradient (gogp_cg_lml_gradient), the part that needs no GPU: the numpy reference of
tests/cg_lml_ref.py against itself and against dense numpy linear algebra, the host's quadrature routine (hook
gogp_test_cg_quadrature) against a dense eigh, the binding tables, and the refusals of the C call, the hooks and the Python
layer, which validate before they touch a device.

  1  cg_block_hist in float64 returns cg_ref.cg_block's bits, so cg_ref stays the one statement of the iteration; its
     history reproduces the iteration (x_m = sum_k a_k p_k is not stored, so: T from (a, beta) has the Ritz values of the
     preconditioned matrix inside its spectrum);
  2  orthogonal probes (t = N + rank_used, Xi = sqrt(t) Q) make the estimator exact: log|K^| against slogdet to 1e-12
     relative, W against alpha alpha^T - K^^-1 to cond tol, the gradient against the dense 1/2 tr(W dK^);
  3  the quadrature hook against eigh for m = 1, 2, 37 and 300 (coefficients of a real CG run and random ones), to
     16 m u of the sum of the terms' magnitudes;
  4  the float64 reduction inside the long-double reference's bound.
Reference counterpart: none."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cg_lml_ref as L
import cg_ref as C
import gram_ref as R
from gogp_amd import _lib

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_history_block_is_cg_refs_block():                                                                 # 1
    p = C.problem("matern52_2d")
    rng = np.random.default_rng(11)
    B = rng.standard_normal((5, p["N"]))
    B[2] = 0.0
    P, _ = C.precond_of(p["K"], p["d"], 64, 0.0)
    want = C.cg_block(p["Kh"], B, P, 1e-8, 1000)
    got = L.cg_block_hist(p["Kh"], B, P, 1e-8, 1000)
    assert np.array_equal(got["X"].view(np.uint64), want["X"].view(np.uint64))
    assert np.array_equal(got["iterations"], want["iterations"]) and np.array_equal(got["converged"], want["converged"])
    assert got["a"].shape == (int(want["iterations"].max()), 5) and got["iterations"][2] == 0 and got["rho0"][2] == 0
    assert np.array_equal(got["W"], P.apply(B))
    # the Ritz values of column 0 lie inside the spectrum of P^-1/2 K^ P^-1/2
    m = int(got["iterations"][0])
    lam = np.linalg.eigvalsh(L.tridiagonal(got["a"][:m, 0], got["beta"][:m, 0], m))
    Pm = p["K"] * 0
    Pd = (P.Ls / P.dis[:, None]) @ (P.Ls / P.dis[:, None]).T + np.diag(p["d"])
    Lc = np.linalg.cholesky(Pd)
    M = np.linalg.solve(Lc, np.linalg.solve(Lc, p["Kh"]).T)
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert ev[0] * (1 - 1e-8) <= lam[0] and lam[-1] <= ev[-1] * (1 + 1e-8) and Pm.shape == M.shape
    # a frozen column's coefficients are zero from its count on
    for c in range(5):
        assert not got["a"][int(got["iterations"][c]):, c].any()


@pytest.mark.parametrize("key", list(L.ORTHO))
def test_orthogonal_probes_make_the_estimator_exact(key):                                                  # 2
    name, N, rank = L.ORTHO[key]
    p = L.small_problem(name, N)
    _, used = C.precond_of(p["K"], p["d"], rank, 1e-8)
    Xi = L.orthogonal_xi(N + used, 0)
    tol = 1e-10
    e, d = L.estimate(p, rank, tol, Xi, piv_tol=1e-8), L.dense(p)
    assert e["converged"].all() and len(e["quad"]) == N + used
    assert abs(e["logdet"] - d["logdet"]) <= 1e-12 * abs(d["logdet"])
    assert abs(e["lml"] - d["lml"]) <= 1e-12 * (abs(d["lml"]) + abs(d["logdet"]))
    Wd = np.outer(d["alpha"], d["alpha"]) - d["Kinv"]
    assert np.abs(e["W"] - Wd).max() <= p["cond"] * tol * np.abs(d["Kinv"]).max()
    floor = (p["cond"] * tol + p["cond"] * N * C.U) * np.abs(d["grad"]).max()
    print(key, "logdet", abs(e["logdet"] - d["logdet"]) / abs(d["logdet"]), "grad", np.abs(e["grad"] - d["grad"]).max(), floor)
    assert (np.abs(e["grad"] - d["grad"]) <= floor).all()


def _cg_coefficients(m):
    """a, beta of m iterations of a real run (Jacobi on the Matern case, tol far below reach, so that it runs on)."""
    p = C.problem("matern32_1d")
    P, _ = C.precond_of(p["K"], p["d"], 0, 0.0)
    z = np.random.default_rng(3).standard_normal((1, p["N"]))
    h = L.cg_block_hist(p["Kh"], z, P, 1e-300, m)
    assert h["iterations"][0] == m
    return h["a"][:, 0].copy(), h["beta"][:, 0].copy(), float(h["rho0"][0])


@pytest.mark.parametrize("m", [1, 2, 37, 300])
def test_quadrature_hook_against_eigh(m):                                                                  # 3
    _lib.build()
    from gogp_amd import gp
    rng = np.random.default_rng([7, m])
    sets = [(rng.uniform(0.2, 2.0, m), rng.uniform(0.01, 0.9, m), 1.7), _cg_coefficients(m)]
    for a, beta, rho0 in sets:
        lam, V = np.linalg.eigh(L.tridiagonal(a, beta, m))
        want = rho0 * float((V[0] ** 2 * np.log(lam)).sum())
        mag = abs(rho0) * float((V[0] ** 2 * np.abs(np.log(lam))).sum())
        # both are backward stable eigensolvers of the same T: eigenvalues to m u |T|, so log lambda to m u cond(T)
        cond = lam[-1] / lam[0]
        got = gp.cg_quadrature(a, beta, rho0)
        assert abs(got - want) <= 16 * m * C.U * (mag + abs(rho0) * cond), (m, got, want)
        assert got == gp.cg_quadrature(a, beta, rho0)
    assert gp.cg_quadrature(np.zeros(0), np.zeros(0), 3.0) == 0.0
    with pytest.raises(ValueError):
        gp.cg_quadrature(np.ones(3), np.ones(2), 1.0)


def test_quadrature_of_a_diagonal_and_of_a_known_matrix():
    _lib.build()
    from gogp_amd import gp
    # m = 1: log(1 / a) rho0
    assert gp.cg_quadrature(np.array([0.25]), np.array([0.0]), 2.0) == 2.0 * np.log(4.0)
    # beta = 0 decouples: e_1^T log(T) e_1 = log T_11 whatever follows
    got = gp.cg_quadrature(np.array([0.5, 0.1, 3.0]), np.array([0.0, 0.0, 0.0]), 1.0)
    assert abs(got - np.log(2.0)) <= 4 * C.U


@pytest.mark.parametrize("case", [("normal", 3), ("max_terms", 3), ("ard", 17), ("periodic", 1)], ids=str)
def test_float64_reduction_inside_its_bound(case):                                                         # 4
    kp = R.kp_of((case[0], case[1], 0, 0))
    rng = np.random.default_rng([98, case[1]])
    n, S = 70, 5
    X, A, B = rng.uniform(-1, 1, (n, case[1])), rng.standard_normal((S, n)), rng.standard_normal((S, n))
    want, bound = L.slot_sums_ab(kp, X, n, A, B, -0.25)
    got, _ = L.slot_sums_ab(kp, X, n, A, B, -0.25, mode="f64")
    assert (np.abs(got.astype(np.longdouble) - want).astype(float) <= bound).all()
    assert bound.max() <= 1e-9 * float((np.abs(0.25 * A).T @ np.abs(B)).sum()) * sum(abs(T["c"]) for T in kp.terms)


def test_the_golden_file_holds_every_case():
    with open(os.path.join(ROOT, "tests", "golden", "cg_lml.json")) as f:
        g = json.load(f)
    assert set(g["ortho"]) == set(L.ORTHO) and set(g["random"]) == set(C.SMALL)
    for name, e in g["random"].items():
        assert abs(e["ref_sigmas"]) <= 3.0 and len(e["grad_diff"]) == len(C.CASES[name][3]), name  # chosen seeds: within 3
    for key, e in g["ortho"].items():
        assert e["N"] == L.ORTHO[key][1] and e["rank"] == L.ORTHO[key][2] and len(e["grad_err"]) == len(C.CASES[L.ORTHO[key][0]][3])


# ---- bindings ------------------------------------------------------------------------------------------------------------------
def test_symbols_bound_and_declared():
    """Fails without the feature: gogp_cg_lml_gradient and the three hooks are in the binding's tables with the headers'
    argument counts, the headers declare them and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_cg_lml_gradient": 11}
    want_hooks = {"gogp_test_cg_grad": 14, "gogp_test_cg_probes": 15, "gogp_test_cg_quadrature": 5, "gogp_test_cg_dots": 19}

    def header(name):
        with open(os.path.join(ROOT, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    h, hh = header("gogp_hip.h"), header("gogp_testhooks.h")
    for tab, text, names in ((table, h, want), (hooks, hh, want_hooks)):
        for name, nargs in names.items():
            assert name in tab and len(tab[name][1]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
    assert ctypes.sizeof(_lib.CCgLmlInfo) == 56 and ctypes.sizeof(_lib.CCgCol) == 24 and ctypes.sizeof(_lib.CCgInfo) == 24
    assert _lib.CCgLmlInfo.logdet_stderr.offset == 32 and _lib.CCgLmlInfo.probes.offset == 40
    assert _lib.CCgLmlInfo.lanczos_max.offset == 52
    m = re.search(r"typedef struct \{([^}]*)\} gogp_cg_lml_info;", h)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("double lml, yt_alpha, logdet, logdet_precond, logdet_stderr; "
                                                             "int32_t probes, blocks, products, lanczos_max;")
    with open(os.path.join(ROOT, "include", "gogp_hip.h")) as f:
        raw = f.read()
    assert "Out of scope: the log-determinant" not in raw and "the log-determinant is not computed" not in raw
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    assert lib.gogp_cg_lml_gradient is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None
    import gogp_amd
    from gogp_amd import gp
    for name in ("CGObserve", "CGGradient"):
        assert callable(getattr(gp.GP, name))
    assert gogp_amd.CGModel is gp.CGModel and "1 / sqrt(probes)" in gp.CGModel.__doc__ and "Adam" in gp.CGModel.__doc__
    for name in ("cg_grad_check", "cg_probes_check", "cg_quadrature"):
        assert callable(getattr(gp, name))


def test_c_abi_refuses_a_null_handle():
    _lib.build()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    info, col = _lib.CCgLmlInfo(), (_lib.CCgCol * 1)()
    assert _lib.lib().gogp_cg_lml_gradient(None, dp, 1, 1, 1e-8, 10, dp, 1, dp, ctypes.byref(info), col) == EARG


# ---- the hooks refuse bad arguments before they touch a device (device = -1) ----------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _grad(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D, n, S, ld = 2, g("n", 10), g("S", 3), g("ld", 12)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    X = np.zeros(g("x_len", 10 * D))
    A, B = np.zeros(g("a_len", 2 * 12 + 10)), np.zeros(g("b_len", 2 * 12 + 10))
    return gp.cg_grad_check(kp, X, n, A, B, ld, S, np.zeros(g("out_len", gp.NACC)), scale=g("scale", 1.0))


GRAD_REFUSED = [dict(n=0), dict(S=0), dict(S=257), dict(ld=9), dict(x_len=19), dict(a_len=33), dict(b_len=33), dict(kind=7),
                dict(events=((0.0, 1.0, 0.5),)), dict(scale=float("nan")), dict(n=(1 << 16) + 1)]


@pytest.mark.parametrize("bad", GRAD_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in GRAD_REFUSED])
def test_grad_hook_refuses(gpm, bad):
    with pytest.raises(gpm.GogpError) as e:
        _grad(gpm, **bad)
    assert e.value.code == EARG


def test_hooks_refuse_and_pass_on(gpm):
    with pytest.raises(ValueError):
        _grad(gpm, out_len=gpm.NACC - 1)
    try:
        out = _grad(gpm)
    except gpm.GogpError as e:
        assert e.code == EHIP  # a well-formed call gets as far as the device
    else:
        assert out.shape == (gpm.NACC,)
    n, r, T, ld = 10, 3, 2, 12
    ok = dict(Ls=np.zeros(2 * 11 + 10), ldn=11, d=np.ones(n), Xi=np.zeros(14 + 13), ldxi=14, Z=np.zeros(ld + n))
    call = lambda **k: gpm.cg_probes_check(k.get("Ls", ok["Ls"]), k.get("ldn", 11), k.get("n", n), k.get("r", r),  # noqa: E731
                                           k.get("d", ok["d"]), k.get("Xi", ok["Xi"]), k.get("ldxi", 14), k.get("ld", ld),
                                           k.get("T", T), k.get("Z", ok["Z"]))
    for bad in (dict(n=0), dict(T=0), dict(T=65), dict(r=-1), dict(r=1025), dict(ldxi=12), dict(Xi=np.zeros(14 + 12)),
                dict(Z=np.zeros(ld + n - 1)), dict(ld=9), dict(d=np.ones(n - 1)), dict(ldn=9), dict(Ls=np.zeros(2 * 11 + 9)),
                dict(Ls=None), dict(r=0)):
        with pytest.raises(gpm.GogpError) as e:
            call(**bad)
        assert e.value.code == EARG, bad
    try:
        assert call().shape == (ld + n,)
    except gpm.GogpError as e:
        assert e.code == EHIP


def test_python_layer_validates(gpm):
    """CGObserve's own checks come before the library is asked (a handle cannot be made without a device, so the
    checks are read off a bare object)."""
    g = object.__new__(gpm.GP)
    g._cg_n, g.NDim = 5, 1
    with pytest.raises(ValueError):
        gpm.GP.CGObserve(g, [0.0], probes=0)
    with pytest.raises(ValueError):
        gpm.GP.CGObserve(g, [0.0], rank=-1)
    with pytest.raises(ValueError):
        gpm.GP.CGObserve(g, [0.0], probes=2, rank=3, xi=np.zeros((2, 7)))   # N + rank = 8 columns at least
    with pytest.raises(ValueError):
        gpm.GP.CGObserve(g, [0.0], probes=2, rank=3, xi=np.zeros((3, 8)))   # probes rows
    with pytest.raises(gpm.GogpError):
        gpm.GP.CGGradient(g)
    a = gpm.GP._cg_normals(5, 7, 2, 3)
    assert a.shape == (3, 9) and gpm.GP._cg_normals(5, 7, 2, 3) is a and not a.flags.writeable
    assert np.array_equal(a, np.random.default_rng(5).standard_normal((3, 9)))
