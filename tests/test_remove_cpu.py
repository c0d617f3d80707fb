"""gogp_remove without a GPU: compaction + the orthogonal rank-m update (tests/remove_ref.py) stays inside the GPU test's
tolerances against the oracle's Absorb of the kept rows, on the GPU test's own inputs; GP.Remove checks its arguments
before the library is called; and the entry point is declared, exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import append_ref as A
import remove_ref as R
from gogp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", R.SHAPES + [R.REPLACED, R.UNTOUCHED, R.AFTER_OBSERVE, R.RESTORED], ids=R.shape_id)
def test_update_matches_oracle_absorb_of_the_kept_rows(shape):
    from oracle.oracle import Oracle
    n, idx, fam = shape
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    X, y, Z = R.inputs(n, D)
    kept = R.kept_of(n, idx)
    o = Oracle(D, simil, noise)
    o.Absorb(X, y, ts, tn)
    L1, alpha, lml = R.state_after_remove(o.L, y, idx)
    if len(kept) == 0:
        assert L1.shape == (0, 0) and lml == 0.0
        return
    o1 = Oracle(D, simil, noise)
    o1.Absorb(X[kept], y[kept], ts, tn)
    A.assert_state(lml, alpha, L1, o1.LML(), o1.Alpha, o1.L, R.shape_id(shape))
    first = min(idx)
    np.testing.assert_array_equal(L1[:first], o.L[:first][:, kept])  # rows above the first removed one keep their bits


def test_last_row_removed_is_the_leading_block():
    from oracle.oracle import Oracle
    D, simil, noise, ts, tn = A.FAMILIES["matern32"]
    X, y, _ = A.inputs(257, D)
    o = Oracle(D, simil, noise)
    o.Absorb(X, y, ts, tn)
    np.testing.assert_array_equal(R.remove_update(o.L, (256,)), o.L[:256, :256])


def test_sliding_window_stays_inside_the_tolerance():
    from oracle.oracle import Oracle
    n, steps, fam = R.SLIDING
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    X, y, _ = A.inputs(n + steps, D)
    o = Oracle(D, simil, noise)
    o.Absorb(X, y, ts, tn)
    K = o.K
    L = np.linalg.cholesky(K[:n, :n])
    for s in range(steps):
        L1 = R.remove_update(L, (0,))
        Kw = K[s + 1:s + n + 1, s + 1:s + n + 1]
        L = np.zeros((n, n))  # the newest row joins as gogp_append's block update does
        L[:n - 1, :n - 1] = L1
        l21 = np.linalg.solve(L1, Kw[n - 1, :n - 1])
        L[n - 1, :n - 1] = l21
        L[n - 1, n - 1] = np.sqrt(Kw[n - 1, n - 1] - l21 @ l21)
    o1 = Oracle(D, simil, noise)
    o1.Absorb(X[steps:], y[steps:], ts, tn)
    np.testing.assert_allclose(L, o1.L, rtol=1e-8, atol=1e-10)


class _Stub:
    def __init__(self):
        self.calls = []

    def gogp_remove(self, h, idx, m):
        self.calls.append([idx[i] for i in range(m)])
        return _lib.GOGP_OK


def _bare_gp(n):
    from gogp_amd.gp import GP
    g = GP.__new__(GP)
    g.NDim = 2
    g._h = ctypes.c_void_p()
    g._X = np.arange(2.0 * n).reshape(n, 2)
    g._Y = np.arange(float(n))
    g._data_dirty = False
    g._with_obs = True
    return g


def test_python_layer_checks_its_arguments_before_the_library(monkeypatch):
    from gogp_amd.gp import GP, GogpError
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    g = _bare_gp(6)
    for bad in ([6], [-1], [2, 2], [0, 5, 0]):
        with pytest.raises(ValueError):
            g.Remove(bad)
    with pytest.raises(TypeError):
        g.Remove([1.5])
    assert stub.calls == [] and len(g.Y) == 6
    g.Remove([])
    assert stub.calls == [] and g._with_obs
    g.Remove(iter((4, 1)))  # any iterable, sorted here
    assert stub.calls == [[1, 4]]
    np.testing.assert_array_equal(g.Y, [0.0, 2.0, 3.0, 5.0])
    np.testing.assert_array_equal(g.X[:, 0], [0.0, 4.0, 6.0, 10.0])
    assert not g._with_obs
    g.Y = g.Y  # assigned since the last Absorb: the device no longer holds them
    with pytest.raises(GogpError) as ei:
        g.Remove([0])
    assert ei.value.code == _lib.GOGP_ESTATE and stub.calls == [[1, 4]]
    g._h = None  # nothing to destroy
    assert callable(getattr(GP, "Remove"))


def test_remove_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+gogp_remove\s*\(\s*gogp_handle\s*\*\s*h\s*,\s*const\s+int64_t\s*\*", hdr)
    _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gogp_remove")
    assert "gogp_remove" in {name for name, _, _ in _lib.SYMBOLS}
    assert _lib.lib().gogp_remove.argtypes[-1] is ctypes.c_int64
    src = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    assert "int Remove(const std::vector<int64_t> &idx)" in src and "gogp_remove(" in src
    go = open(os.path.join(ROOT, "go", "gogp", "gp.go")).read()
    assert "func (gp *GP) Remove(idx []int)" in go and "C.gogp_remove(" in go
