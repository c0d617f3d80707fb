"""gogp_append without a GPU: the block update itself (tests/append_ref.py) stays inside the GPU test's tolerances
against the oracle's Absorb of all observations, on the GPU test's own inputs; and the entry point is declared,
exported and bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import append_ref as A
from gogp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", A.SHAPES + [A.RESTORED, A.REPEATED], ids=A.shape_id)
def test_block_update_matches_oracle_absorb(shape):
    from oracle.oracle import Oracle
    n, m, fam = shape
    D, simil, noise, ts, tn = A.FAMILIES[fam]
    X, y, Z = A.inputs(n + m, D)
    o = Oracle(D, simil, noise)
    o.Absorb(X, y, ts, tn)
    chunk = 1 if shape == A.REPEATED else A.CHUNK
    L, alpha, lml = A.block_append(o.K, y, n, chunk)
    A.assert_state(lml, alpha, L, o.LML(), o.Alpha, o.L, shape)


def test_append_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gogp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+gogp_append\s*\(\s*gogp_handle\s*\*", hdr)
    _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gogp_append")
    assert "gogp_append" in {name for name, _, _ in _lib.SYMBOLS}
    assert _lib.lib().gogp_append.argtypes[-1] is ctypes.c_int64


def test_python_layer_checks_its_arguments_before_the_device():
    from gogp_amd.gp import GP
    assert callable(getattr(GP, "Append"))
    src = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    assert "int Append(" in src and "gogp_append(" in src
    go = open(os.path.join(ROOT, "go", "gogp", "gp.go")).read()
    assert "func (gp *GP) Append(x [][]float64, y []float64)" in go and "C.gogp_append(" in go
