"""GP.Append (gogp_append) on the GPU: Absorb(X[:n]) then Append(X[n:], y[n:]) against the oracle's Absorb(X, y) on LML,
Alpha, L and Produce, at the tolerances of tests/test_gpu_parity.py::_check_against; the rollback, the refusals, the
events kernel and the C++ mirror.  Shapes and inputs: tests/append_ref.py (tests/test_append_cpu.py shows on the CPU
that the update itself stays inside these tolerances on them)."""
import os
import subprocess

import numpy as np
import pytest

import append_ref as A
import events_ref as R
from gogp_amd import _lib, kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _oracle(shape):
    """The oracle's Absorb of all n + m rows of a shape: computed once, shared, read only."""
    if shape not in _ORACLE:
        from oracle.oracle import Oracle
        n, m, fam = shape
        D, simil, noise, ts, tn = A.FAMILIES[fam]
        X, y, Z = A.inputs(n + m, D)
        o = Oracle(D, simil, noise)
        o.Absorb(X, y, ts, tn)
        _ORACLE[shape] = (X, y, Z, o.LML(), o.Alpha, o.L, o.Produce(Z), o)
    return _ORACLE[shape]


def _gp(fam, **kw):
    from gogp_amd.gp import GP
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    return GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, device=0, **kw)


def _compare(g, shape):
    X, y, Z, lml_o, alpha_o, L_o, (mu_o, sg_o), _ = _oracle(shape)
    assert len(g.Y) == len(y) and int(_lib.lib().gogp_n(g._h)) == len(y)
    A.assert_state(g.LML(), g.Alpha, g.L, lml_o, alpha_o, L_o, shape)
    mu, sg = g.Produce(Z)
    A.assert_produce(mu, sg, mu_o, sg_o, shape)


@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_append_matches_absorb_of_all(shape):
    n, m, fam = shape
    X, y = _oracle(shape)[:2]
    g = _gp(fam)
    if n:
        g.Absorb(X[:n], y[:n])
    g.Append(X[n:], y[n:])
    np.testing.assert_array_equal(g.X, X)
    _compare(g, shape)
    g.close()


def test_append_after_restore_recomputes_z():
    n, m, fam = A.RESTORED
    X, y = _oracle(A.RESTORED)[:2]
    src = _gp(fam)
    src.Absorb(X[:n], y[:n])
    g = _gp(fam)
    g.X, g.Y = X[:n], y[:n]
    g.restore(src.L, src.Alpha)
    g.Append(X[n:], y[n:])
    _compare(g, A.RESTORED)
    src.close()
    g.close()


def test_repeated_single_appends():
    n, m, fam = A.REPEATED
    X, y = _oracle(A.REPEATED)[:2]
    g = _gp(fam)
    g.Absorb(X[:n], y[:n])
    for i in range(n, n + m):
        g.Append(X[i:i + 1], y[i:i + 1])
        assert int(_lib.lib().gogp_n(g._h)) == i + 1
    _compare(g, A.REPEATED)
    g.close()


def test_events_on_both_sides_of_a_boundary():
    from gogp_amd.gp import GP
    events = [(-0.5, 0.3, 0.5), (0.9, 1.4, 0.3)]
    rng = np.random.default_rng(5)
    n, m = 120, 20
    X = rng.uniform(-2.0, 2.0, (n + m, 1))
    y = np.sin(2.0 * X[:, 0]) + 0.3 * X[:, 0] + 0.1 * rng.normal(size=n + m)
    new = X[n:, 0]
    assert (new < -0.5).any() and ((new > 0.3) & (new < 0.9)).any() and (new > 1.4).any()
    th = [1.5, 0.8, 1.2]  # noise std 0.1 * 1.2
    r = R.RefGP(1, events)
    r.X, r.Y = X, y
    lml_r = r.Observe(np.log(th))
    g = GP(1, kernel.Events(kernel.Scaled(kernel.Matern52), events, 0), kernel.ScaledNoise(0.01), ThetaSimil=th[:2],
           ThetaNoise=th[2:], device=0)
    g.Absorb(X[:n], y[:n])
    g.Append(X[n:], y[n:])
    A.assert_state(g.LML(), g.Alpha, g.L, lml_r, r.alpha, r.L, "events")
    Z = np.array([[-1.0], [-0.5], [0.0], [0.3], [0.6], [1.4], [1.9]])
    A.assert_produce(*g.Produce(Z), *r.Produce(Z), "events")
    g.close()


def test_observe_then_append_then_observe():
    shape = (300, 64, "ard_rbf3")
    n, m, fam = shape
    X, y, Z, _, _, _, _, o = _oracle(shape)
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    x = np.log(np.array(list(ts) + list(tn)))
    g = _gp(fam)
    g.X, g.Y = X[:n], y[:n]
    g.Observe(x)  # eager: the inverse is still running when Append starts
    g.Append(X[n:], y[n:])
    _compare(g, shape)
    with pytest.raises(Exception) as ei:
        g.Gradient()
    assert ei.value.code == _lib.GOGP_ESTATE
    from oracle.oracle import Oracle
    o2 = Oracle(D, simil, noise)
    o2.set_data(X, y)
    lml, lml_o = g.Observe(x), o2.Observe(x)
    assert abs(lml - lml_o) <= 1e-8 * max(1.0, abs(lml_o))
    grad, grad_o = g.Gradient(), o2.Gradient()
    assert np.abs(grad - grad_o).max() <= 1e-6 * max(1.0, np.abs(grad_o).max()), (grad, grad_o)
    g.close()


@pytest.mark.parametrize("second_chunk", [False, True], ids=["m1", "m70"])
def test_rollback_is_exact(second_chunk):
    from gogp_amd.gp import GP, FactorizeError
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0], device=0)
    X0, y0 = np.array([[0.0], [1.0]]), np.array([1.0, 0.0])
    if second_chunk:
        # the duplicate of x = 0 as the second of 70 rows (two chunks: 64 + 6), the others well separated
        far = 3.0 + 2.5 * np.arange(69)
        Xa = np.concatenate([[[far[0]]], [[0.0]], far[1:69, None]])
        ya = np.concatenate([[0.5], [1.0], np.linspace(-1, 1, 68)])
        assert len(ya) == 70
        pivot = 3
    else:
        Xa, ya, pivot = np.array([[0.0]]), np.array([1.0]), 2
    g.Absorb(X0, y0)
    Z = np.array([[0.25], [0.5], [1.5]])
    mu0, sg0 = g.Produce(Z)
    L0, a0, lml0 = g.L, g.Alpha, g.LML()
    with pytest.raises(FactorizeError) as ei:
        g.Append(Xa, ya)
    assert ei.value.pivot == pivot
    assert len(g.Y) == 2 and int(_lib.lib().gogp_n(g._h)) == 2
    mu1, sg1 = g.Produce(Z)
    assert np.array_equal(mu0, mu1) and np.array_equal(sg0, sg1)
    assert np.array_equal(L0, g.L) and np.array_equal(a0, g.Alpha) and lml0 == g.LML()
    g.close()


def test_rollback_covers_earlier_chunks():
    """The duplicate as row 65 of a 70-row append: it fails in the second chunk, the pivot is global, and the 64 rows
    of the first chunk are rolled back too."""
    from gogp_amd.gp import GP, FactorizeError
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0], device=0)
    g.Absorb([[0.0], [1.0]], [1.0, 0.0])
    Z = np.array([[0.25], [0.5], [1.5]])
    mu0, sg0 = g.Produce(Z)
    L0 = g.L
    far = 3.0 + 2.5 * np.arange(69)
    Xa = np.concatenate([far[:64, None], [[far[64]]], [[0.0]], far[65:69, None]])
    ya = np.linspace(-1, 1, 70)
    with pytest.raises(FactorizeError) as ei:
        g.Append(Xa, ya)
    assert ei.value.pivot == 2 + 65
    assert len(g.Y) == 2 and int(_lib.lib().gogp_n(g._h)) == 2
    mu1, sg1 = g.Produce(Z)
    assert np.array_equal(mu0, mu1) and np.array_equal(sg0, sg1) and np.array_equal(L0, g.L)
    g.close()


def test_refusals():
    from gogp_amd.gp import GP, GogpError
    D, simil, noise, ts, tn = A.FAMILIES["scaled_rbf3"]
    X, y, Z = A.inputs(40, D)
    g32 = GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, device=0, precision=32)
    g32.Absorb(X[:30], y[:30])
    with pytest.raises(GogpError) as ei:
        g32.Append(X[30:], y[30:])
    assert ei.value.code == _lib.GOGP_EARG and "precision" in str(ei.value)
    g32.close()
    g = GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, X=X[:30], Y=y[:30], device=0)
    with pytest.raises(GogpError) as ei:
        g.Append(X[30:], y[30:])  # nothing absorbed
    assert ei.value.code == _lib.GOGP_ESTATE
    g._push_data()  # the same through the C ABI: data set, not factored
    rc = _lib.lib().gogp_append(g._h, X[30:].ctypes.data_as(_lib._dp), y[30:].ctypes.data_as(_lib._dp), 10)
    assert rc == _lib.GOGP_ESTATE
    g.Absorb(X[:30], y[:30])
    mu0, sg0 = g.Produce(Z)
    bad = y[30:].copy()
    bad[3] = np.nan
    with pytest.raises(GogpError) as ei:
        g.Append(X[30:], bad)
    assert ei.value.code == _lib.GOGP_EARG
    assert len(g.Y) == 30
    mu1, sg1 = g.Produce(Z)
    assert np.array_equal(mu0, mu1) and np.array_equal(sg0, sg1)
    with pytest.raises(ValueError):
        g.Append(X[30:], y[31:])
    g.Append(X[30:30], y[30:30])  # m = 0: nothing happens
    assert len(g.Y) == 30
    g.close()


def test_cpp_mirror(tmp_path):
    _lib.build()
    exe = str(tmp_path / "cpp_append_driver")
    libdir = os.path.join(ROOT, "gogp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp_append_driver.cpp"), "-o", exe,
                           "-L" + libdir, "-lgogp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    shape = (250, 7, "matern32")
    X, y, Z, lml_o, alpha_o, L_o, (mu_o, sg_o), _ = _oracle(shape)
    D, simil, noise, ts, tn = A.FAMILIES["matern32"]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (250, 7, len(Z)))
        f.write("%.17g %.17g %.17g\n" % (ts[0], ts[1], tn[0]))
        for v in list(X[:, 0]) + list(y) + list(Z[:, 0]):
            f.write("%.17g\n" % v)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.array([float(v) for v in r.stdout.split()])
    n = 257
    assert out.size == 1 + n + n * n + 2 * len(Z)
    A.assert_state(out[0], out[1:1 + n], out[1 + n:1 + n + n * n].reshape(n, n), lml_o, alpha_o, L_o, "cpp")
    A.assert_produce(out[1 + n + n * n:1 + n + n * n + len(Z)], out[1 + n + n * n + len(Z):], mu_o, sg_o, "cpp")
