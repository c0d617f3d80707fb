"""Vecchia's approximation (gogp_vecchia_*), the part that needs no GPU: the binding tables, the refusals the C calls and
the hook make before they touch a device, gogp_vecchia_check on hand-made tables, the table helpers of
gogp_amd/vecchia.py against naive loops, and the references of tests/vecchia_ref.py held to each other, to dense numpy
and to the golden file.

Reference counterpart: none."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import gram_ref as R
import grad_reduce_ref as G
import vecchia_ref as V
from gogp_amd import _lib
from gogp_amd import vecchia as VT

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_tables():
    """Fails without the feature: the five gogp_vecchia_* symbols and the hook are in the binding's tables with the
    headers' argument counts, the headers declare them and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_vecchia_check": 5, "gogp_vecchia_set_data": 7, "gogp_vecchia_observe": 5, "gogp_vecchia_gradient": 3,
            "gogp_vecchia_produce": 6}
    want_hooks = {"gogp_test_vecchia": 26, "gogp_test_vecchia_blocks": 2}

    def header(name):
        with open(os.path.join(ROOT, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    h, hh = header("gogp_hip.h"), header("gogp_testhooks.h")
    for tab, text, names in ((table, h, want), (hooks, hh, want_hooks)):
        for name, nargs in names.items():
            assert name in tab and len(tab[name][1]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
    assert "#define GOGP_VECCHIA_MAX_M 63" in h and _lib.GOGP_VECCHIA_MAX_M == 63 == VT.MAX_M
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None
    import gogp_amd
    from gogp_amd import gp
    for name in ("SetVecchia", "VecchiaObserve", "VecchiaTerms", "VecchiaGradient", "VecchiaProduce"):
        assert callable(getattr(gp.GP, name))
    assert callable(gp.vecchia_check) and gogp_amd.VecchiaModel is gp.VecchiaModel and gogp_amd.vecchia is VT
    src = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    for name in want:
        assert name + "(" in src, name


def test_register_budget_of_the_kernel():
    """The instances meet the audit's limits through two devices the compiler could undo (vecchia.hip: the parameters
    re-read per pair, the data pointers kept in vector registers).  Built here they stand at 125 / 152 / 170 / 113 VGPRs
    and 4 / 30 / 35 / 4 SGPR spills (value / gradient / ARD pass / produce); the audit fails at 256 and 48.  This fails
    earlier -- at 200 and 42, a fifth above today's worst -- so that a drift shows before the limit is reached."""
    import sys
    _lib.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_audit
    ks = [k for k in codeobj_audit.kernels(_lib.LIB_PATH) if "vecchia_kernel" in k["name"]]
    assert len(ks) == 8, [k["name"] for k in ks]
    for k in ks:
        assert k["vgpr_count"] <= 200 and k.get("sgpr_spill_count", 0) <= 42, (k["name"], k["vgpr_count"], k.get("sgpr_spill_count"))
        assert not k.get("agpr_count", 0) and not k.get("vgpr_spill_count", 0) and not k.get("private_segment_fixed_size", 0)


def _i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_c_abi_refuses_a_null_handle():
    _lib.build()
    L = _lib.lib()
    one, t = np.zeros(1), np.full(1, -1, np.int32)
    dp = one.ctypes.data_as(_lib._dp)
    assert L.gogp_vecchia_set_data(None, dp, dp, None, 1, _i32p(t), 1) == EARG
    assert L.gogp_vecchia_observe(None, dp, 1, dp, None) == EARG
    assert L.gogp_vecchia_gradient(None, dp, 1) == EARG
    assert L.gogp_vecchia_produce(None, dp, 1, _i32p(t), dp, None) == EARG


def check(table, n=None, causal=True):
    t = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    rows, m = t.shape
    return _lib.lib().gogp_vecchia_check(_i32p(t) if t.size else None, rows, m, rows if n is None else n, int(causal))


def test_check_on_hand_made_tables():
    _lib.build()
    good = [[-1, -1], [0, -1], [1, 0], [0, 2]]
    assert check(good) == OK
    assert check([[-1, -1], [0, -1], [2, 0], [0, 2]]) == EARG, "not causal: row 2 names itself"
    assert check([[-1, -1], [0, -1], [3, 0], [0, 2]]) == EARG, "not causal: row 2 names a later row"
    assert check([[-1, -1], [0, -1], [1, 1], [0, 2]]) == EARG, "duplicate"
    assert check([[-1, -1], [0, -1], [1, 0], [0, 4]], causal=False) == EARG, "out of range"
    assert check([[-1, -1], [0, -1], [1, 0], [0, -2]]) == EARG, "a negative index that is not -1"
    assert check([[-1, -1], [0, -1], [-1, 0], [0, 2]]) == EARG, "-1 in the middle"
    assert check([[0, -1], [0, -1], [1, 0], [0, 2]]) == EARG, "row 0 is not empty"
    assert check([[3, 1], [0, 2], [3, 0], [2, 3]], causal=False) == OK, "produce: every index in [0, n)"
    assert check([[3, 1]], n=3, causal=False) == EARG
    assert check(np.full((3, 64), -1)) == EARG, "m = 64"
    assert check(np.full((3, 63), -1)) == OK
    assert check(np.zeros((3, 0))) == OK, "m = 0"
    assert check(np.zeros((0, 5))) == OK, "no rows"
    assert check(good, n=3) == EARG, "more causal rows than observations"
    assert _lib.lib().gogp_vecchia_check(None, 3, 2, 3, 1) == EARG, "NULL table"
    assert check(V.all_earlier(64)) == OK
    assert check(VT.previous(100, 7)) == OK


# ---- the table helpers -------------------------------------------------------------------------------------------------
def naive_nearest(x, z, m, lengths, earlier):
    xs = x / lengths if lengths is not None else x
    zs = xs if z is None else (z / lengths if lengths is not None else z)
    out = np.full((len(zs), m), -1, np.int32)
    for i in range(len(zs)):
        lim = i if earlier else len(xs)
        d2 = [sum((zs[i, d] - xs[j, d]) ** 2 for d in range(xs.shape[1])) for j in range(lim)]
        order = sorted(range(lim), key=lambda j: (d2[j], j))[:m]
        out[i, :len(order)] = order
    return out


def test_previous():
    for n, m in ((0, 3), (1, 3), (5, 0), (6, 2), (4, 7), (70, 63)):
        t = VT.previous(n, m)
        assert t.shape == (n, m) and t.dtype == np.int32
        for i in range(n):
            want = [i - 1 - k for k in range(m) if i - 1 - k >= 0]
            assert list(t[i, :len(want)]) == want and (t[i, len(want):] == -1).all()
        assert check(t) == OK
    with pytest.raises(ValueError):
        VT.previous(5, 64)


@pytest.mark.parametrize("lengths", [None, (0.5, 2.0)])
def test_nearest_against_a_naive_loop_with_ties(lengths):
    """Points on an integer grid (with repeats): most distances tie, and ties go to the lower index."""
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (60, 2)).astype(float)
    z = rng.integers(0, 4, (17, 2)).astype(float)
    ln = None if lengths is None else np.array(lengths)
    for m in (0, 1, 5, 63):
        for chunk in (7, 1024):
            t = VT.nearest(x, m, ln, chunk=chunk)
            assert np.array_equal(t, naive_nearest(x, None, m, ln, True)), (m, chunk)
            assert check(t) == OK
            tz = VT.nearest_to(x, z, m, ln, chunk=chunk)
            assert np.array_equal(tz, naive_nearest(x, z, m, ln, False)), (m, chunk)
            assert check(tz, n=60, causal=False) == OK
    x1 = rng.uniform(0, 1, 30)  # a 1-d array is N x 1
    assert np.array_equal(VT.nearest(x1, 4), naive_nearest(x1.reshape(-1, 1), None, 4, None, True))


# ---- the references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "matern52", "periodic", "max_terms", "ard"])
def test_the_identity_against_two_dense_solves(kind):
    """The first reference (rank-two identity) against the second (LML(c + i) - LML(c) and the difference of the dense
    gradients), both in float64: N = 40, D = 2, random tables of m = 7 with per-observation variances.  The blocks'
    condition numbers are below 1e3 (unit scale, noise variance 0.05), so 1e-11 of the quantity's size is a hundred
    times what rounding leaves."""
    kp = G.KP(2, R.terms_of(kind, 2), noise_var=0.05)
    X, y, v = V.inputs(1, 40, 2)
    t = V.random_table(np.random.default_rng(7), 40, 7, 40)
    a = V.observe(kp, X, y, v, t, "f64")
    logp, value, slots = V.observe_dense(kp, X, y, v, t)
    assert not a["failed"]
    assert np.abs(a["terms"][:, 2] - logp).max() <= 1e-11 * np.abs(logp).max()
    assert abs(a["value"] - value) <= 1e-11 * abs(value)
    assert np.abs(a["slots"] - slots).max() <= 1e-11 * np.abs(slots).max()
    assert np.abs(slots).max() > 0


def test_all_earlier_rows_give_the_dense_lml():
    """c(i) = every earlier row at N = 48: the value is the dense LML (slogdet, solve), the slot sums those of
    W = alpha alpha^T - K^-1, mu_i / s_i the sequential forecasts."""
    kp = G.KP(2, R.terms_of("matern32", 2), noise_var=0.05)
    X, y, v = V.inputs(2, 48, 2)
    a = V.observe(kp, X, y, v, V.all_earlier(48), "f64")
    K = R.pair_values(kp, X, X, "f64")[0] + np.diag(kp.noise_var + v)
    sign, logdet = np.linalg.slogdet(K)
    alpha = np.linalg.solve(K, y)
    lml = -0.5 * y @ alpha - 0.5 * logdet - 24 * np.log(2 * np.pi)
    assert sign > 0 and abs(a["value"] - lml) <= 1e-11 * abs(lml)
    want = V.slots_of(kp, X, np.outer(alpha, alpha) - np.linalg.inv(K), np.float64)
    assert np.abs(a["slots"] - want).max() <= 1e-10 * np.abs(want).max()
    i = 30
    ks = K[i, :i]
    assert abs(a["terms"][i, 0] - ks @ np.linalg.solve(K[:i, :i], y[:i])) <= 1e-11
    assert abs(a["terms"][i, 1] ** 2 - (K[i, i] - ks @ np.linalg.solve(K[:i, :i], ks))) <= 1e-11


def test_gradient_is_the_derivative_of_the_value():
    """The reference's gradient against central differences of its own value in long double (step 1e-6: truncation 1e-12
    of the third derivative, rounding 1e-19 / 1e-6), every component, the noise parameter's included."""
    p = V.golden_problem("nearest-N200-m7")
    X, y, t = p["X"][:60], p["y"][:60], p["t"][:60]

    def value(x):
        th = np.exp(x)
        return V.observe(G.kp_from_desc(p["desc"], th[:-1], th[-1:]), X, y, None, t, "ld", grad=False)["value"]

    a = V.observe(p["kp"], X, y, None, t, "ld")
    grad = V.gradient_of(p, a["slots"])
    for k in range(len(p["x"])):
        e = np.zeros(len(p["x"]))
        e[k] = 1e-6
        fd = (value(p["x"] + e) - value(p["x"] - e)) / np.longdouble(2e-6)
        assert abs(fd - grad[k]) <= 1e-8 * max(1.0, abs(grad[k])), (k, fd, grad[k])


def test_produce_reference_against_dense():
    kp = G.KP(2, R.terms_of("normal", 2), noise_var=0.05)
    X, y, v = V.inputs(3, 40, 2)
    Z = np.random.default_rng(1).uniform(-2, 2, (5, 2))
    tz = np.tile(np.arange(40, dtype=np.int32)[::-1], (5, 1))
    mu, sigma, failed = V.produce(kp, X, y, v, Z, tz, "f64")
    K = R.pair_values(kp, X, X, "f64")[0] + np.diag(kp.noise_var + v)
    ks = R.pair_values(kp, Z, X, "f64")[0]
    assert not failed
    assert np.abs(mu - ks @ np.linalg.solve(K, y)).max() <= 1e-11
    assert np.abs(sigma ** 2 - (R.prior_values(kp) - np.einsum("ij,ji->i", ks, np.linalg.solve(K, ks.T)))).max() <= 1e-11


def test_golden_cases_are_well_conditioned_and_current():
    """On every golden case the reference meets no pivot that is not positive, and the file's value, the magnitudes of the
    terms and mu are what the reference computes here -- to 1e-9 of their size: another numpy build may add in another
    order."""
    with open(os.path.join(ROOT, "tests", "golden", "vecchia.json")) as f:
        gold = json.load(f)
    assert gold["noise_std"] == V.GOLDEN_NOISE_STD >= 0.05 and set(gold["cases"]) == set(V.GOLDEN)
    for name in V.GOLDEN:
        p, c = V.golden_problem(name), gold["cases"][name]
        a = V.observe(p["kp"], p["X"], p["y"], p["v"], p["t"], "f64", grad=False)
        mu, sigma, failed = V.produce(p["kp"], p["X"], p["y"], p["v"], p["Z"][:5], p["tz"][:5], "f64")
        assert not a["failed"] and not failed, name
        assert gogp_check(p["t"]) and gogp_check(p["tz"], p["N"], False), name
        assert abs(a["value"] - c["value"]) <= 1e-9 * abs(c["value"]), name
        assert np.abs(np.abs(a["terms"]).max(0) - np.array(c["terms_norm"])).max() <= 1e-9 * max(c["terms_norm"]), name
        assert abs(a["terms"][:, 2].sum() - c["value"]) <= 1e-9 * abs(c["value"]) and len(c["grad"]) == len(p["x"]), name
        assert "mu" not in c or np.abs(mu - np.array(c["mu"][:5])).max() <= 1e-9, name


def gogp_check(t, n=None, causal=True):
    return check(t, n, causal) == OK


# ---- the hook refuses bad arguments before it touches a device ----------------------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def test_hook_refuses_bad_arguments_and_passes_good_ones_on(gpm):
    kp = G.KP(2, R.terms_of("normal", 2), noise_var=0.05)
    X, y, v = V.inputs(4, 8, 2)
    t = V.random_table(np.random.default_rng(3), 8, 3, 8)

    def call(**kw):
        a = dict(X=X.reshape(-1).copy(), y=y.copy(), v=None, n=8, nbr=np.ascontiguousarray(t.reshape(-1)), m=3,
                 terms=np.zeros(24), partials=np.zeros(8 * G.NACC), vpart=np.zeros(8), Z=None, targets=None, max_blocks=0)
        a.update(kw)
        try:
            gpm.vecchia_check(kp.hook(gpm), a["X"], a["y"], a["v"], a["n"], a["nbr"], a["m"], a["terms"], a["partials"],
                              a["vpart"], Z=a["Z"], targets=a["targets"], max_blocks=a["max_blocks"])
        except gpm.GogpError as e:
            return e.code
        return OK

    bad = t.copy()
    bad[3, 0] = 3
    assert call(nbr=np.ascontiguousarray(bad.reshape(-1))) == EARG, "a table that is not causal"
    assert call(n=9) == EARG and call(m=64) == EARG and call(m=4) == EARG
    assert call(terms=np.zeros(23)) == EARG and call(partials=np.zeros(8 * G.NACC - 1)) == EARG and call(vpart=np.zeros(7)) == EARG
    assert call(v=np.zeros(7)) == EARG and call(max_blocks=-1) == EARG and call(targets=5) == EARG
    assert call(Z=np.zeros(4), targets=2, terms=np.zeros(4)) == EARG, "produce takes no partials"
    assert gpm.vecchia_blocks(5) == 5 and gpm.vecchia_blocks(10 ** 6) == 2048 and gpm.vecchia_blocks(200, 7) == 7
    assert call() in (OK, EHIP), "a well-formed call gets as far as the device"
    tz = V.random_table(np.random.default_rng(4), 2, 3, 8, causal=False)
    assert call(Z=np.zeros(4), targets=2, terms=np.zeros(4), partials=None, vpart=None,
                nbr=np.ascontiguousarray(tz.reshape(-1))) in (OK, EHIP)
