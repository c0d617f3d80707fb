"""The schedules the defaults select by size, and the fp32 path, at ragged N against the CPU oracle (run with -m gpu).

With no option set the library picks its launch schedule from npad (N rounded up to 256; gogp_amd/csrc/api.hip):

    superpanel_head   head super-panels 3 panels wide (fp64) / 4 (fp32)       npad > 4096   superpanel_width
    chain_prio        chain launches lose their raised priority               npad > 6144   chain_prio_of
    chain_split       panel128 chain step -> 256-block kernel beside the      npad > 8192   chain_split_of
                      inverse (Absorb keeps form 2)
    graph = 2         the explicit candidates graph gives way to the streams  npad > 8192   GRAPH_EXPLICIT_MAX_NPAD
    kinv_fused        K^-1 becomes an unfused LAUUM in two launches           npad > 10240  factorize_t, kinv_split

Every mechanism has a test that forces it through its option at n = 300 / 2300; here the DEFAULT schedule runs at
N = 4400, 6200, 8100, 8300, 10200, 10300, 12345 -- none a multiple of 256, one on each side of every switch
(tests/cases.py: REGIME_SIZES) -- against oracle.FastOracle:

  * LML, and every gradient component ON ITS OWN SCALE, |g_p - o_p| <= tol_p |o_p| (no oracle component may be below
    1e-4 of the largest: that would be a cancellation).  The tolerances are measured, not chosen: 100 x what two
    independent oracle variants differ by on that case (tests/golden/schedule_regimes.json, written by
    tests/golden/make_schedule_regimes.py), capped by the suite's 1e-9 (LML) and 1e-7 (gradient);
  * Alpha, Produce for m = 1, 64 (trsm_small.hip), 65 (first size of the tile route) and 300; the same after Absorb;
  * the WHOLE factor: |L L^T - K|_ij <= rho gamma_{n+1} (|L||L|^T)_ij elementwise (Higham), K from the oracle's Gram
    build; rho <= min(1, 8 rho_ref) with rho_ref what LAPACK's own factor reaches on that case.  One wrong tile or
    padding row anywhere fails it;
  * a second evaluation bit for bit; one handle walked across the regimes (stale buffers, a stale kinv_c1);
  * the launch record shows that the regime ran (a K = 768 bulk update; two LAUUM launches above npad 10240);
  * precision = 32 at N = 129 .. 8300 under the fp32 contract of DESIGN.md section 6, gradient_precision = 32 at
    8300 / 10300, candidates at 4400 (graph 1, 2) and 8300 (streams) bit-equal to single calls.

The tests pin results, not one schedule: forcing the other side of a switch must pass the same assertions.

Measured on an MI355X (this module's own printout; `tol` is the bound of that case):

    case             LML rel (tol)          worst gradient component, rel to itself (tol)   factor rho (bound)
    matern52-4400    1.6e-13 (2.8e-12)      grad[0]  4.4e-10 (3.9e-09)                    0.0112 (0.0317)
    matern52-6200    9.7e-14 (4.4e-12)      grad[2]  2.8e-13 (1.2e-11)                    0.0082 (0.0251)
    matern52-8100    2.0e-13 (1.6e-11)      grad[2]  4.5e-13 (3.5e-11)                    0.0061 (0.0246)
    matern52-8300    1.1e-13 (4.0e-12)      grad[0]  7.7e-09 (1.0e-07)                    0.0062 (0.0263)
    matern52-10200   3.9e-14 (8.6e-12)      grad[1]  1.1e-10 (4.9e-09)                    0.0051 (0.0141)
    matern52-10300   1.4e-14 (6.2e-12)      grad[1]  4.6e-09 (1.0e-07)                    0.0050 (0.0212)
    matern52-12345   1.2e-14 (3.8e-12)      grad[0]  1.2e-09 (1.0e-07)                    0.0043 (0.0180)
    ard_rbf9-8300    2.1e-14 (9.8e-13)      grad[7]  1.4e-13 (3.0e-12)                    0.0058 (0.0164)
    ard_rbf9-10300   2.9e-14 (6.9e-13)      grad[4]  2.1e-13 (6.5e-13)                    0.0052 (0.0244)
    hyperpriors-4400 5.2e-15 (1.1e-12)      grad[2]  9.4e-12 (4.1e-10)                    0.0119 (0.0426)

    fp32 case        LML rel   gradient of max|g|   alpha     mu m=40   sigma m=40   (bounds: see test_fp32_path_at_ragged_sizes)
    config5-129      8.4e-08   5.9e-08              2.1e-11   2.8e-06   3.7e-06
    config5-257      7.7e-08   7.3e-08              5.2e-10   5.3e-06   7.7e-06
    config5-700      1.5e-07   1.6e-07              5.3e-08   1.2e-05   1.9e-05
    config5-2300     1.6e-07   2.1e-07              3.7e-07   3.4e-05   3.0e-05
    config5-4400     1.7e-07   2.3e-07              1.1e-06   6.5e-05   2.3e-05
    config5-8300     1.8e-07   2.8e-07              2.7e-06   8.1e-05   2.0e-05
    config3-129      6.2e-08   3.9e-08              1.2e-10   6.3e-06   1.2e-05
    config3-257      6.0e-08   4.6e-08              1.1e-09   9.0e-06   2.1e-05
    config3-700      2.1e-07   1.5e-07              1.2e-07   1.7e-05   6.3e-05
    config3-2300     3.7e-07   1.9e-07              7.0e-07   1.5e-05   9.4e-05
    config3-4400     6.0e-07   2.9e-07              2.1e-06   2.8e-05   1.1e-04
    config3-8300     1.1e-06   4.9e-07              3.4e-06   2.8e-05   1.0e-04

    gradient_precision = 32, N = 8300: gradient 4.9e-07 of max|g| (bound 1e-6), LML bit-identical
    gradient_precision = 32, N = 10300: gradient 4.9e-07 of max|g| (bound 1e-6), LML bit-identical
    alpha / mu / sigma (fp64, every case, Observe and Absorb): at most 3.4e-04 of their rtol 1e-6 + atol 1e-8 criterion
"""
import functools
import json
import math
import os

import numpy as np
import pytest

from cases import (REGIME_CASES, REGIME_FAMILIES, REGIME_M, REGIME_SIZES, REGIME_THRESHOLDS, factor_residual_ratio,
                   regime_inputs)

pytestmark = pytest.mark.gpu

LML_CAP, GRAD_CAP, MARGIN = 1e-9, 1e-7, 100.0   # the suite's bounds; the margin over the oracle variants' disagreement
MIN_COMPONENT_RATIO = 1e-4
PRODUCE_M = (1, 64, 65, REGIME_M)


@pytest.fixture(scope="module")
def gpmod():
    from gogp_amd import gp
    return gp


@functools.lru_cache(maxsize=None)
def _record():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_regimes.json")
    with open(path) as f:
        return {(c["family"], c["n"]): c for c in json.load(f)["cases"]}


def _npad(n):
    return -(-n // 256) * 256


def _regime(npad):
    """Which side of every switch a padded size is on."""
    return {k: npad > v for k, v in REGIME_THRESHOLDS.items()}


class _Figures:
    """Prints every figure before anything is asserted (a failing run still reports all of them)."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def le(self, name, value, bound):
        ok = bool(value <= bound)   # NaN fails
        print("REGIME %-28s %-22s %.3e  (bound %.3e)%s" % (self.tag, name, value, bound, "" if ok else "  FAIL"),
              flush=True)
        if not ok:
            self.bad.append((name, value, bound))

    def close_to(self, name, got, want, rtol, atol):
        """np.testing.assert_allclose's criterion, reported as the largest |got - want| / (atol + rtol |want|)."""
        got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
        assert got.shape == want.shape, (self.tag, name, got.shape, want.shape)
        self.le(name, float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))), 1.0)

    def done(self):
        assert not self.bad, (self.tag, self.bad)


@functools.lru_cache(maxsize=None)
def _oracle_case(family, n):
    """FastOracle() on one case: the vectors only (the factor is dropped; the oracle object stays for its Gram build)."""
    from oracle.oracle import FastOracle
    D, simil, noise, _, _, _ = REGIME_FAMILIES[family]
    X, y, Z, x = regime_inputs(family, n)
    o = FastOracle(D, simil, noise)
    o.set_data(X, y)
    lml = o.Observe(x)
    mu, sigma = o.Produce(Z)
    d = np.diag(o.Lc)
    out = {"lml": lml, "alpha": o.Alpha.copy(), "mu": mu, "sigma": sigma, "cond_diag": float((d.max() / d.min()) ** 2),
           "oracle": o}
    out["grad"] = o.Gradient()
    o.Lc = None
    return out


def _tolerances(family, n):
    rec = _record()[(family, n)]
    tol_lml = min(LML_CAP, MARGIN * rec["lml_disagreement"])
    tol_grad = np.minimum(GRAD_CAP, MARGIN * np.array(rec["grad_disagreement"]))
    return rec, tol_lml, tol_grad


def _check_inputs(family, n):
    rec = _record()[(family, n)]
    X, y, Z, x = regime_inputs(family, n)
    assert X.sum() == rec["x_sum"] and y.sum() == rec["y_sum"] and Z.sum() == rec["z_sum"], (family, n)
    assert x.tolist() == rec["log_theta"]
    return X, y, Z, x


def _new_gp(gpmod, family, X, y, **kw):
    D, simil, noise, _, _, _ = REGIME_FAMILIES[family]
    return gpmod.GP(D, simil, noise, X=X, Y=y, **kw)


def _check_values(fig, ref, tol_lml, tol_grad, lml, grad, prefix=""):
    fig.le(prefix + "lml rel", abs(lml - ref["lml"]) / abs(ref["lml"]), tol_lml)
    if grad is not None:
        go = ref["grad"]
        for p in range(len(go)):
            fig.le(prefix + "grad[%d] rel own" % p, abs(grad[p] - go[p]) / abs(go[p]), tol_grad[p])


def _check_state(fig, g, ref, Z, prefix=""):
    ao = ref["alpha"]
    fig.close_to(prefix + "alpha", g.Alpha, ao, 1e-6, 1e-8 * np.abs(ao).max())
    for m in PRODUCE_M:
        mu, sigma = g.Produce(Z[:m])
        fig.close_to(prefix + "mu m=%d" % m, mu, ref["mu"][:m], 1e-6, 1e-8)
        fig.close_to(prefix + "sigma m=%d" % m, sigma, ref["sigma"][:m], 1e-6, 1e-8)


def _check_factor(fig, g, ref, rho_ref, prefix=""):
    o = ref["oracle"]
    K = o._gram(o.ts, o.tn)
    L = g.L
    assert L.shape == K.shape
    rho, at = factor_residual_ratio(L, K)
    print("REGIME %-28s %-22s tile (%d, %d) of 256, entry %s" % (fig.tag, prefix + "largest residual at",
                                                                   at[0] // 256, at[1] // 256, at), flush=True)
    fig.le(prefix + "factor rho", rho, min(1.0, 8.0 * rho_ref))


#: (lml, gradient) of a fresh handle with default options per case, filled by the test below
_FRESH = {}


def _fresh(gpmod, family, n):
    if (family, n) not in _FRESH:
        X, y, _, x = regime_inputs(family, n)
        g = _new_gp(gpmod, family, X, y)
        _FRESH[(family, n)] = (g.Observe(x), g.Gradient())
        g.close()
    return _FRESH[(family, n)]


def test_case_table_lands_on_both_sides_of_every_switch():
    """The sizes are where the table says, ragged, and every switch has a size on each side."""
    sides = {k: set() for k in REGIME_THRESHOLDS}
    for n, (npad, panels) in REGIME_SIZES.items():
        assert n % 256 != 0 and _npad(n) == npad and npad // 256 == panels
        for k, above in _regime(npad).items():
            sides[k].add(above)
    assert all(s == {False, True} for k, s in sides.items() if k != "superpanel_head"), sides
    assert sides["superpanel_head"] == {True}   # every size has head super-panels; 4096 and below: test_gpu_parity
    r = {n: _regime(npad) for n, (npad, _) in REGIME_SIZES.items()}
    assert r[6200]["chain_prio"] and not r[4400]["chain_prio"]
    assert not r[8100]["chain_split"] and r[8300]["chain_split"] and r[8300]["graph_explicit"]
    assert not r[10200]["kinv_fused"] and r[10300]["kinv_fused"] and r[12345]["kinv_fused"]
    # 18 panels: one head super-panel of 3 (more than 16 to come), then width 2 with a 1-panel tail
    assert REGIME_SIZES[4400][1] == 18 and (18 - 3) % 2 == 1


@pytest.mark.parametrize("family,n", REGIME_CASES, ids=["%s-%d" % c for c in REGIME_CASES])
def test_default_schedule_against_oracle(gpmod, family, n):
    """Section by section what the module docstring lists, for one (family, N) on a handle with no option set."""
    X, y, Z, x = _check_inputs(family, n)
    rec, tol_lml, tol_grad = _tolerances(family, n)
    ref = _oracle_case(family, n)
    fig = _Figures("%s-%d" % (family, n))
    go = ref["grad"]
    # the condition under which a component's own value is its scale
    ratio = np.abs(go).min() / np.abs(go).max()
    print("REGIME %-28s oracle gradient %s  min/max %.2e  (max L_ii / min L_ii)^2 %.1f" % (
        fig.tag, go, ratio, ref["cond_diag"]), flush=True)
    assert ratio >= MIN_COMPONENT_RATIO, (family, n, go)
    g = _new_gp(gpmod, family, X, y)
    lml, grad = g.Observe(x), g.Gradient()
    _FRESH[(family, n)] = (lml, grad)
    _check_values(fig, ref, tol_lml, tol_grad, lml, grad)
    _check_state(fig, g, ref, Z)
    _check_factor(fig, g, ref, rec["rho_ref"])
    # the second evaluation on the handle: bit for bit
    lml2, grad2 = g.Observe(x), g.Gradient()
    fig.le("second evaluation |dlml|", abs(lml2 - lml), 0.0)
    fig.le("second evaluation |dgrad|", float(np.abs(grad2 - grad).max()), 0.0)
    g.close()
    # Absorb: the lazy path (no gradient preparation; chain form 2 at every size)
    D, simil, noise, ts, tn, _ = REGIME_FAMILIES[family]
    ga = gpmod.GP(D, simil, noise, ThetaSimil=list(np.exp(x[:len(ts)])), ThetaNoise=list(np.exp(x[len(ts):])))
    ga.Absorb(X, y)
    _check_values(fig, ref, tol_lml, tol_grad, ga.LML(), None, prefix="absorb ")
    _check_state(fig, ga, ref, Z, prefix="absorb ")
    if _regime(_npad(n))["chain_split"]:   # a chain other than the eager sweep's: its whole factor as well
        _check_factor(fig, ga, ref, rec["rho_ref"], prefix="absorb ")
    ga.close()
    fig.done()


def test_one_handle_walked_across_the_regimes(gpmod):
    """Stale buffers and a stale kinv_c1: ONE handle takes the sizes in an order that crosses every switch in both
    directions -- first a factorisation above npad 10240 whose early K^-1 launch no Gradient picks up -- and returns at
    every step, bit for bit, what a fresh handle returns (which the test above holds against the oracle); Produce and
    Absorb in between."""
    family = "matern52"
    fig = _Figures("walk")
    X, y, Z, x = regime_inputs(family, 10300)
    g = _new_gp(gpmod, family, X, y)
    fig.le("10300 observe only |dlml|", abs(g.Observe(x) - _fresh(gpmod, family, 10300)[0]), 0.0)
    for step, n in enumerate((4400, 12345, 8300, 10300, 8100, 10200, 6200, 10300)):
        X, y, Z, x = regime_inputs(family, n)
        ref = _oracle_case(family, n)
        _, tol_lml, tol_grad = _tolerances(family, n)
        lml0, grad0 = _fresh(gpmod, family, n)
        if step == 2:   # a lazy factorisation in between: Absorb, Produce, no gradient
            g.ThetaSimil, g.ThetaNoise = list(np.exp(x[:2])), list(np.exp(x[2:]))
            g.Absorb(X, y)
            _check_values(fig, ref, tol_lml, tol_grad, g.LML(), None, prefix="%d absorb " % n)
            mu, sigma = g.Produce(Z[:65])
            fig.close_to("%d absorb mu m=65" % n, mu, ref["mu"][:65], 1e-6, 1e-8)
            fig.close_to("%d absorb sigma m=65" % n, sigma, ref["sigma"][:65], 1e-6, 1e-8)
        g.X, g.Y = X, y
        lml, grad = g.Observe(x), g.Gradient()
        fig.le("%d |dlml| to fresh" % n, abs(lml - lml0), 0.0)
        fig.le("%d |dgrad| to fresh" % n, float(np.abs(grad - grad0).max()), 0.0)
        _check_values(fig, ref, tol_lml, tol_grad, lml, grad, prefix="%d " % n)
        mu, sigma = g.Produce(Z[:64])
        fig.close_to("%d mu m=64" % n, mu, ref["mu"][:64], 1e-6, 1e-8)
        fig.close_to("%d sigma m=64" % n, sigma, ref["sigma"][:64], 1e-6, 1e-8)
        fig.close_to("%d alpha" % n, g.Alpha, ref["alpha"], 1e-6, 1e-8 * np.abs(ref["alpha"]).max())
    g.close()
    fig.done()


def _launch_tags(g):
    _, _, _, tag = g.profile_read_launches()
    return tag // 100000000, (tag % 100000000) // 100000   # mode (common.h: GemmMode), K / 16


@pytest.mark.parametrize("n", sorted(REGIME_SIZES))
def test_launch_record_shows_the_regime(gpmod, n):
    """The tile kernel's launch record (tag = mode, K / 16, tiles) of one Observe + Gradient with no option set: a bulk
    update of the trailing matrix (lower tiles, mode 1) with K = 768, i.e. a head super-panel 3 panels wide; above npad
    10240 K^-1 = Y Y^T as two LAUUM launches (mode 2; the first inside the sweep, option kinv_split), at and below it
    none at all: the sweep accumulates K^-1 panel by panel (mode 1), and no separate launch follows.  The recorded
    evaluation returns the bits of the unrecorded one."""
    family = "matern52"
    X, y, _, x = regime_inputs(family, n)
    regime = _regime(_npad(n))
    g = _new_gp(gpmod, family, X, y)
    g.profile_enable(True)
    lml, grad = g.Observe(x), g.Gradient()
    mode, k16 = _launch_tags(g)
    g.profile_read()
    g.profile_enable(False)
    g.close()
    lauum = int((mode == 2).sum())
    head = int(((mode == 1) & (k16 == 768 // 16)).sum())
    print("REGIME launches-%d: %d launches, %d lower-tile launches with K = 768, %d LAUUM" % (n, len(mode), head, lauum))
    assert regime["superpanel_head"] and head >= 1, (n, head, sorted(set(k16.tolist())))
    assert lauum == (2 if regime["kinv_fused"] else 0), (n, lauum)
    lml0, grad0 = _fresh(gpmod, family, n)
    assert lml == lml0
    np.testing.assert_array_equal(grad, grad0)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 path and mixed gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 257, 700, 2300, 4400, 8300])
@pytest.mark.parametrize("shape", ["config5", "config3"])
def test_fp32_path_at_ragged_sizes(gpmod, shape, n):
    """precision = 32 (float matrices, fp32 MFMA products; fp64 diagonal blocks via diagsyrk.hip, refinement of alpha
    against the exact Gram matrix: kmatvec_kernel) with a partially filled last panel, and at 4400 / 8300 with its head
    super-panels 4 panels wide, against the fp64 oracle under the bounds of the fp32 contract as
    test_fp32_path_accuracy_contract states them: config-5 shape LML 2e-6, gradient 2e-5 of
    max|g|, config-3 shape 1e-5 and 1e-4; alpha 2e-5, mu 1e-3, sigma 2e-4 of their largest values.  The LML is also
    rebuilt on the host from the downloaded diagonal of the factor and y^T alpha; Produce for m = 7 and m = 40."""
    from gogp_amd import configs
    from oracle.oracle import FastOracle
    wl = configs.workload(5 if shape == "config5" else 3, n)
    X, y = wl.inputs()
    assert len(y) == n and n % 256 != 0
    Z = wl.test_points(40)
    x = wl.log_theta(0)
    o = FastOracle(wl.D, wl.simil, wl.noise)
    o.set_data(X, y)
    lml_o = o.Observe(x)
    mu_o, sg_o = o.Produce(Z)
    alpha_o = o.Alpha.copy()
    logdiag_o = float(np.log(np.diag(o.Lc)).sum())
    grad_o = o.Gradient()
    fig = _Figures("fp32-%s-%d" % (shape, n))
    tol_lml, tol_grad = (2e-6, 2e-5) if shape == "config5" else (1e-5, 1e-4)
    g = gpmod.GP(wl.D, wl.simil, wl.noise, X=X, Y=y, precision=32)
    if _npad(n) > 4096:
        g.profile_enable(True)
    lml, grad = g.Observe(x), g.Gradient()
    if _npad(n) > 4096:   # the head width of the fp32 path: a bulk update with K = 1024
        mode, k16 = _launch_tags(g)
        g.profile_read()
        g.profile_enable(False)
        assert int(((mode == 1) & (k16 == 1024 // 16)).sum()) >= 1, (n, sorted(set(k16.tolist())))
    fig.le("lml rel", abs(lml - lml_o) / abs(lml_o), tol_lml)
    fig.le("grad of max|g|", float(np.abs(grad - grad_o).max() / np.abs(grad_o).max()), tol_grad)
    alpha = g.Alpha
    fig.le("alpha of max", float(np.abs(alpha - alpha_o).max() / np.abs(alpha_o).max()), 2e-5)
    d = g.L_diag()
    assert d.shape == (n,) and np.all(d > 0)
    lml_host = -0.5 * n * math.log(2 * math.pi) - float(np.log(d).sum()) - 0.5 * float(y @ alpha)
    fig.le("host lml rel to oracle", abs(lml_host - lml_o) / abs(lml_o), tol_lml)
    fig.le("host lml rel to library", abs(lml_host - lml) / abs(lml_o), tol_lml)
    fig.le("log-det part of |lml|", abs(float(np.log(d).sum()) - logdiag_o) / abs(lml_o), tol_lml)
    for m in (7, 40):
        mu, sg = g.Produce(Z[:m])
        fig.le("mu m=%d of max" % m, float(np.abs(mu - mu_o[:m]).max() / np.abs(mu_o[:m]).max()), 1e-3)
        fig.le("sigma m=%d of max" % m, float(np.abs(sg - sg_o[:m]).max() / np.abs(sg_o[:m]).max()), 2e-4)
    # a second evaluation on the handle, as test_fp32_path_accuracy_contract holds it
    fig.le("second evaluation lml rel", abs(g.Observe(x) - lml) / abs(lml), 1e-12)
    g.close()
    fig.done()


@pytest.mark.parametrize("n", [8300, 10300])
def test_mixed_gradient_above_the_chain_split_size(gpmod, n):
    """gradient_precision = 32 above npad 8192, where it takes branches of its own (chain_split_of keeps form 2, K^-1
    fuses at every size): the LML is the fp64 handle's bit for bit, the gradient within the documented 1e-6 of the
    oracle's largest component (include/gogp_hip.h), alpha and Produce stay fp64."""
    family = "matern52"
    X, y, Z, x = regime_inputs(family, n)
    ref = _oracle_case(family, n)
    fig = _Figures("mixed-%d" % n)
    g = _new_gp(gpmod, family, X, y)
    g.set_option("gradient_precision", 32)
    lml, grad = g.Observe(x), g.Gradient()
    fig.le("|dlml| to fp64 handle", abs(lml - _fresh(gpmod, family, n)[0]), 0.0)
    fig.le("grad of max|g|", float(np.abs(grad - ref["grad"]).max() / np.abs(ref["grad"]).max()), 1e-6)
    fig.close_to("alpha", g.Alpha, ref["alpha"], 1e-6, 1e-8 * np.abs(ref["alpha"]).max())
    mu, sigma = g.Produce(Z[:65])
    fig.close_to("mu m=65", mu, ref["mu"][:65], 1e-6, 1e-8)
    fig.close_to("sigma m=65", sigma, ref["sigma"][:65], 1e-6, 1e-8)
    fig.le("second evaluation |dlml|", abs(g.Observe(x) - lml), 0.0)
    g.set_option("gradient_precision", 64)   # and back: the fp64 gradient of a fresh handle
    lml3, grad3 = g.Observe(x), g.Gradient()
    fig.le("back to 64 |dlml|", abs(lml3 - _fresh(gpmod, family, n)[0]), 0.0)
    fig.le("back to 64 |dgrad|", float(np.abs(grad3 - _fresh(gpmod, family, n)[1]).max()), 0.0)
    g.close()
    fig.done()


# ---------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,graph", [(4400, 1), (4400, 2), (8300, 2)])
def test_candidates_bit_equal_to_single_calls(gpmod, n, graph):
    """observe_gradient_candidates with k = 3: at N = 4400 under graph = 1 (a captured chain is for npad <= 1024: the
    streams run) and graph = 2 (the explicitly built graph, replayed from the second identical use), at N = 8300 beyond
    the explicit graph's limit, where graph = 2 falls back to the streams.  Every bit equals single Observe + Gradient
    calls, as include/gogp_hip.h promises; the first candidate is the oracle-checked point of the case table; the
    handle's own factorisation is untouched afterwards."""
    family = "matern52"
    X, y, Z, x = regime_inputs(family, n)
    k = 3
    xs_of = lambda r: x[None, :] + 0.02 * ((np.arange(k)[:, None] + r) % 4) * np.array([1.0, -1.0, 0.5])[None, :]
    g = _new_gp(gpmod, family, X, y)
    want = [[(g.Observe(xc), g.Gradient()) for xc in xs_of(r)] for r in range(3)]
    lml_own, grad_own = g.Observe(x + 0.05), g.Gradient()   # the handle's own state before the batches
    mu_own, sigma_own = g.Produce(Z[:9])
    alpha_own = g.Alpha
    g.set_option("graph", graph)
    for r in range(3):
        lmls, grads, st = g.observe_gradient_candidates(xs_of(r))
        assert list(st) == [0] * k
        for c in range(k):
            assert lmls[c] == want[r][c][0], (r, c, lmls[c], want[r][c][0])
            np.testing.assert_array_equal(grads[c], want[r][c][1])
    nodes, refused = g.graph_info()
    assert not refused
    if graph == 2 and not _regime(_npad(n))["graph_explicit"]:
        assert nodes > 40, nodes      # the explicit graph ran
    else:
        assert nodes == 0, nodes      # the stream path ran
    lml0, grad0 = _fresh(gpmod, family, n)   # xs_of(0)[0] == x
    assert want[0][0][0] == lml0
    np.testing.assert_array_equal(want[0][0][1], grad0)
    assert g.LML() == lml_own
    np.testing.assert_array_equal(g.Gradient(), grad_own)
    np.testing.assert_array_equal(g.Alpha, alpha_own)
    mu, sigma = g.Produce(Z[:9])
    np.testing.assert_array_equal(mu, mu_own)
    np.testing.assert_array_equal(sigma, sigma_own)
    g.close()
