"""GP.Remove (gogp_remove) on the GPU: Absorb(X, y) then Remove(idx) against the oracle's Absorb(X[kept], y[kept]) on LML,
Alpha, L and Produce, at the tolerances of tests/test_gpu_parity.py::_check_against; the rows that keep their bits, the
states the call may find the handle in, the sliding window, the refusals, determinism and the C++ mirror.  Shapes and
inputs: tests/remove_ref.py (tests/test_remove_cpu.py shows on the CPU that the update itself stays inside these
tolerances on them)."""
import os
import subprocess

import numpy as np
import pytest

import append_ref as A
import events_ref as E
import remove_ref as R
from gogp_amd import _lib, kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def _oracle(fam, X, y, Z, key):
    """The oracle's Absorb of the given rows: computed once per key, shared, read only."""
    if key not in _ORACLE:
        from oracle.oracle import Oracle
        D, simil, noise, ts, tn = A.FAMILIES[fam]
        o = Oracle(D, simil, noise)
        o.Absorb(X, y, ts, tn)
        _ORACLE[key] = (o.LML(), o.Alpha, o.L, o.Produce(Z))
    return _ORACLE[key]


def _kept_oracle(shape):
    n, idx, fam = shape
    X, y, Z = R.inputs(n, A.FAMILIES[fam][0])
    kept = R.kept_of(n, idx)
    return X, y, Z, kept, _oracle(fam, X[kept], y[kept], Z, shape)


def _gp(fam, **kw):
    from gogp_amd.gp import GP
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    return GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, device=0, **kw)


def _compare(g, Xk, yk, Z, ref, tag):
    lml_o, alpha_o, L_o, (mu_o, sg_o) = ref
    assert len(g.Y) == len(yk) and int(_lib.lib().gogp_n(g._h)) == len(yk)
    np.testing.assert_array_equal(g.X, Xk)
    np.testing.assert_array_equal(g.Y, yk)
    A.assert_state(g.LML(), g.Alpha, g.L, lml_o, alpha_o, L_o, tag)
    mu, sg = g.Produce(Z)
    A.assert_produce(mu, sg, mu_o, sg_o, tag)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_remove_matches_absorb_of_the_kept_rows(shape):
    n, idx, fam = shape
    X, y, Z, kept, ref = _kept_oracle(shape)
    g = _gp(fam)
    g.Absorb(X, y)
    g.Remove(idx)
    if len(kept) == 0:  # the empty process; a following Append absorbs
        assert int(_lib.lib().gogp_n(g._h)) == 0 and len(g.Y) == 0 and g.LML() == 0.0
        mu, sg = g.Produce(Z)
        e = _gp(fam)
        e.Absorb(X[:0], y[:0])  # no observations, the same parameters: sigma = sqrt(prior)
        mu_e, sg_e = e.Produce(Z)
        assert np.isfinite(sg_e).all()
        assert np.array_equal(mu, np.zeros(len(Z))) and np.array_equal(sg, sg_e)
        e.close()
        g.Append(X, y)
        _compare(g, X, y, Z, _oracle(fam, X, y, Z, ("all",) + shape), shape)
    else:
        _compare(g, X[kept], y[kept], Z, ref, shape)
        # nothing downstream assumes how the state was produced: the device's own data, factorised again
        D, simil, noise, ts, tn = A.FAMILIES[fam]
        lml = g.Observe(np.log(np.array(list(ts) + list(tn))))
        assert abs(lml - ref[0]) <= 1e-8 * max(1.0, abs(ref[0]))
    g.close()


def test_rows_above_the_first_removed_keep_their_bits():
    for shape in (R.UNTOUCHED, R.REPLACED):
        n, idx, fam = shape
        X, y, Z, kept, ref = _kept_oracle(shape)
        first = min(idx)
        assert first == (200 if shape is R.UNTOUCHED else min(i for i in R.IDX_520 if i > 0))
        g = _gp(fam)
        g.Absorb(X, y)
        L0 = g.L
        g.Remove(idx)
        L1 = g.L
        np.testing.assert_array_equal(L1[:first], L0[:first][:, kept])
        np.testing.assert_array_equal(L1[:first, :first], L0[:first, :first])
        _compare(g, X[kept], y[kept], Z, ref, "untouched")
        g.close()
    g = _gp("matern32")  # the last row alone: the whole factor is the old leading block
    X, y, Z = A.inputs(257, 1)
    g.Absorb(X, y)
    L0 = g.L
    g.Remove([256])
    np.testing.assert_array_equal(g.L, L0[:256, :256])
    g.close()


def test_observe_then_remove_then_observe():
    n, idx, fam = R.AFTER_OBSERVE
    X, y, Z, kept, ref = _kept_oracle(R.AFTER_OBSERVE)
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    x = np.log(np.array(list(ts) + list(tn)))
    g = _gp(fam)
    g.X, g.Y = X, y
    g.Observe(x)  # eager: the inverse is still running when Remove starts
    g.Remove(idx)
    _compare(g, X[kept], y[kept], Z, ref, "after observe")
    with pytest.raises(Exception) as ei:
        g.Gradient()
    assert ei.value.code == _lib.GOGP_ESTATE
    f = _gp(fam)
    f.X, f.Y = X[kept], y[kept]
    lml, lml_f = g.Observe(x), f.Observe(x)
    assert abs(lml - lml_f) <= 1e-8 * max(1.0, abs(lml_f))
    grad, grad_f = g.Gradient(), f.Gradient()
    assert np.abs(grad - grad_f).max() <= 1e-6 * max(1.0, np.abs(grad_f).max()), (grad, grad_f)
    g.close()
    f.close()


def test_remove_after_restore_recomputes_z():
    n, idx, fam = R.RESTORED
    X, y, Z, kept, ref = _kept_oracle(R.RESTORED)
    src = _gp(fam)
    src.Absorb(X, y)
    g = _gp(fam)
    g.X, g.Y = X, y
    g.restore(src.L, src.Alpha)
    g.Remove(idx)
    _compare(g, X[kept], y[kept], Z, ref, "restored")
    src.close()
    g.close()


def test_remove_after_append():
    n, m, idx, fam = R.APPENDED
    X, y, Z = A.inputs(n + m, A.FAMILIES[fam][0])
    kept = R.kept_of(n + m, idx)
    g = _gp(fam)
    g.Absorb(X[:n], y[:n])
    g.Append(X[n:], y[n:])
    g.Remove(idx)
    _compare(g, X[kept], y[kept], Z, _oracle(fam, X[kept], y[kept], Z, R.APPENDED), "appended")
    g.close()


def test_sliding_window():
    n, steps, fam = R.SLIDING
    X, y, Z = A.inputs(n + steps, A.FAMILIES[fam][0])
    g = _gp(fam)
    g.Absorb(X[:n], y[:n])
    for s in range(steps):
        g.Remove([0])
        g.Append(X[n + s:n + s + 1], y[n + s:n + s + 1])
        assert int(_lib.lib().gogp_n(g._h)) == n
    _compare(g, X[steps:], y[steps:], Z, _oracle(fam, X[steps:], y[steps:], Z, R.SLIDING), "sliding")
    f = _gp(fam)
    f.Absorb(X[steps:], y[steps:])
    for a, b in zip(g.ProduceGradient(Z), f.ProduceGradient(Z)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)  # as tests/test_produce_gradient_gpu.py between equivalent paths
    g.close()
    f.close()


def test_events_on_both_sides_of_a_boundary():
    from gogp_amd.gp import GP
    events = [(-0.5, 0.3, 0.5), (0.9, 1.4, 0.3)]
    rng = np.random.default_rng(5)
    n, m = 120, 20
    X = rng.uniform(-2.0, 2.0, (n + m, 1))
    y = np.sin(2.0 * X[:, 0]) + 0.3 * X[:, 0] + 0.1 * rng.normal(size=n + m)
    idx = list(range(3, n + m, 7))
    assert len(idx) == m
    kept = R.kept_of(n + m, idx)
    th = [1.5, 0.8, 1.2]  # noise std 0.1 * 1.2
    r = E.RefGP(1, events)
    r.X, r.Y = X[kept], y[kept]
    lml_r = r.Observe(np.log(th))
    g = GP(1, kernel.Events(kernel.Scaled(kernel.Matern52), events, 0), kernel.ScaledNoise(0.01), ThetaSimil=th[:2],
           ThetaNoise=th[2:], device=0)
    g.Absorb(X, y)
    g.Remove(idx)
    A.assert_state(g.LML(), g.Alpha, g.L, lml_r, r.alpha, r.L, "events")
    Z = np.array([[-1.0], [-0.5], [0.0], [0.3], [0.6], [1.4], [1.9]])
    A.assert_produce(*g.Produce(Z), *r.Produce(Z), "events")
    g.close()


def test_refusals():
    from gogp_amd.gp import GP, GogpError
    L = _lib.lib()
    i64p = L.gogp_remove.argtypes[1]
    D, simil, noise, ts, tn = A.FAMILIES["scaled_rbf3"]
    X, y, Z = A.inputs(40, D)
    g32 = GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, device=0, precision=32)
    g32.Absorb(X, y)
    with pytest.raises(GogpError) as ei:
        g32.Remove([3])
    assert ei.value.code == _lib.GOGP_EARG and "precision" in str(ei.value)
    g32.close()
    g = GP(D, simil, noise, ThetaSimil=ts, ThetaNoise=tn, X=X, Y=y, device=0)
    g._push_data()  # data set, not factored
    one = np.array([3], dtype=np.int64)
    assert L.gogp_remove(g._h, one.ctypes.data_as(i64p), 1) == _lib.GOGP_ESTATE
    g.Absorb(X, y)
    mu0, sg0 = g.Produce(Z)
    L0, a0, lml0 = g.L, g.Alpha, g.LML()
    for bad in ([5, 3], [3, 3], [3, 40], [-1, 3]):  # unsorted, duplicate, out of range: through the C ABI
        arr = np.array(bad, dtype=np.int64)
        assert L.gogp_remove(g._h, arr.ctypes.data_as(i64p), len(arr)) == _lib.GOGP_EARG, bad
    assert L.gogp_remove(g._h, None, 2) == _lib.GOGP_EARG
    assert int(L.gogp_n(g._h)) == 40
    mu1, sg1 = g.Produce(Z)
    assert np.array_equal(mu0, mu1) and np.array_equal(sg0, sg1)
    assert np.array_equal(L0, g.L) and np.array_equal(a0, g.Alpha) and lml0 == g.LML()
    assert L.gogp_remove(g._h, None, 0) == _lib.GOGP_OK  # m = 0: nothing happens
    g.Remove([])
    assert len(g.Y) == 40 and np.array_equal(L0, g.L)
    with pytest.raises(ValueError):
        g.Remove([40])
    g.close()


def test_two_identical_sequences_return_the_same_bits():
    shape = R.SHAPES[-2]
    n, idx, fam = shape
    X, y, Z = A.inputs(n, A.FAMILIES[fam][0])
    out = []
    for _ in range(2):
        g = _gp(fam)
        g.Absorb(X, y)
        g.Remove(idx)
        out.append((g.L, g.Alpha))
        g.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_cpp_mirror(tmp_path):
    _lib.build()
    exe = str(tmp_path / "cpp_remove_driver")
    libdir = os.path.join(ROOT, "gogp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp_remove_driver.cpp"), "-o", exe,
                           "-L" + libdir, "-lgogp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])
    shape = (257, (0,), "matern32")
    n, idx, fam = shape
    X, y, Z, kept, (lml_o, alpha_o, L_o, (mu_o, sg_o)) = _kept_oracle(shape)
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (n, len(idx), len(Z)))
        f.write("%.17g %.17g %.17g\n" % (ts[0], ts[1], tn[0]))
        for v in list(X[:, 0]) + list(y) + list(Z[:, 0]):
            f.write("%.17g\n" % v)
        for i in reversed(idx):  # any order
            f.write("%d\n" % i)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.array([float(v) for v in r.stdout.split()])
    k = len(kept)
    assert out.size == 1 + k + k * k + 2 * len(Z)
    A.assert_state(out[0], out[1:1 + k], out[1 + k:1 + k + k * k].reshape(k, k), lml_o, alpha_o, L_o, "cpp")
    A.assert_produce(out[1 + k + k * k:1 + k + k * k + len(Z)], out[1 + k + k * k + len(Z):], mu_o, sg_o, "cpp")
