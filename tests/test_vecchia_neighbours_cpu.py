"""Neighbour tables built on the device (gogp_vecchia_neighbours and its kin, gogp_amd/csrc/vecchia_knn.hip), the part that
needs no GPU: the binding tables, the refusals made before a device is touched, the plan of the search, the value checks
of the Python methods and the register audit of the new kernels.

Reference counterpart: none."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from gogp_amd import _lib

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 63, 64, 65, 129, 257, 1000]  # the shapes of tests/test_vecchia_knn_kernel.py
MS = [0, 1, 7, 31, 32, 63]
WS_PER_M = 768 * 64 * 12  # include/gogp_testhooks.h: the workspace stays under this many bytes per entry of a row


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def test_binding_tables():
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_vecchia_neighbours": 8, "gogp_vecchia_set_data_nearest": 7, "gogp_vecchia_reneighbour": 2,
            "gogp_vecchia_get_neighbours": 2, "gogp_vecchia_produce_nearest": 7}
    want_hooks = {"gogp_test_vecchia_knn": 18, "gogp_test_vecchia_knn_plan": 4}

    def header(name):
        with open(os.path.join(ROOT, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    h, hh = header("gogp_hip.h"), header("gogp_testhooks.h")
    for tab, text, names in ((table, h, want), (hooks, hh, want_hooks)):
        for name, nargs in names.items():
            assert name in tab and len(tab[name][1]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None
    from gogp_amd import gp
    for name in ("VecchiaNeighbours", "SetVecchiaNearest", "VecchiaReneighbour", "VecchiaNeighbourTable",
                 "VecchiaProduceNearest"):
        assert callable(getattr(gp.GP, name))
    assert callable(gp.VecchiaModel.reneighbour) and callable(gp.vecchia_knn_check) and callable(gp.vecchia_knn_plan)
    src = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    for name in want:
        assert name + "(" in src, name


def test_c_abi_refuses_a_null_handle():
    _lib.build()
    L = _lib.lib()
    one, t = np.ones(1), np.full(1, -1, np.int32)
    dp, tp = one.ctypes.data_as(_lib._dp), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.gogp_vecchia_neighbours(None, dp, 1, None, 0, dp, 1, tp) == EARG
    assert L.gogp_vecchia_set_data_nearest(None, dp, dp, None, 1, dp, 1) == EARG
    assert L.gogp_vecchia_reneighbour(None, dp) == EARG
    assert L.gogp_vecchia_get_neighbours(None, tp) == EARG
    assert L.gogp_vecchia_produce_nearest(None, dp, 1, dp, dp, None, None) == EARG


def test_hook_refuses_bad_arguments_before_the_device(gpm):
    X = np.arange(24, dtype=np.float64)

    def call(**kw):
        a = dict(X=X, n=8, ndim=3, m=2, nbr=np.zeros(16, np.int32), d2=np.zeros(16), xs=np.zeros(24), Z=None, targets=None,
                 lengths=None, slabs=0, tile_cap=0)
        a.update(kw)
        try:
            gpm.vecchia_knn_check(a["X"], a["n"], a["ndim"], a["m"], a["nbr"], a["d2"], a["xs"], Z=a["Z"], targets=a["targets"],
                                  lengths=a["lengths"], slabs=a["slabs"], tile_cap=a["tile_cap"])
        except gpm.GogpError as e:
            return e.code
        return OK

    assert call(n=9) == EARG and call(n=0) == EARG and call(ndim=0) == EARG and call(ndim=65) == EARG
    assert call(m=-1) == EARG and call(m=64) == EARG and call(m=3) == EARG
    assert call(nbr=np.zeros(15, np.int32)) == EARG and call(d2=np.zeros(15)) == EARG and call(xs=np.zeros(23)) == EARG
    assert call(nbr=None) == EARG and call(d2=None) == EARG
    assert call(targets=5) == EARG, "the causal form has a target per row"
    assert call(Z=np.zeros(5), targets=2) == EARG and call(Z=np.zeros(6), targets=9) == EARG
    assert call(slabs=-1) == EARG and call(slabs=257) == EARG and call(tile_cap=-1) == EARG
    assert call(lengths=np.array([1.0, 0.0, 1.0])) == EARG and call(lengths=np.array([1.0, -2.0, 1.0])) == EARG
    assert call(lengths=np.array([1.0, np.inf, 1.0])) == EARG and call(lengths=np.array([1.0, np.nan, 1.0])) == EARG
    assert call(lengths=np.ones(2)) == EARG
    assert call() in (OK, EHIP), "a well-formed call gets as far as the device"
    assert call(Z=np.zeros(6), targets=2, nbr=np.zeros(4, np.int32), d2=np.zeros(4), lengths=np.ones(3), slabs=3) in (OK, EHIP)
    assert call(m=0, nbr=None, d2=None) in (OK, EHIP)
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, -1), (5, 5, 64)):
        with pytest.raises(gpm.GogpError):
            gpm.vecchia_knn_plan(*bad)


def cover(targets, n, tile, slabs):
    """How often every (target, candidate) pair falls into a work unit of the documented geometry."""
    hits = np.zeros((targets, n), dtype=np.int64)
    L = -(-n // slabs)
    for t0 in range(0, targets, tile):
        for s in range(slabs):
            hits[t0:min(targets, t0 + tile), s * L:min(n, (s + 1) * L)] += 1
    return hits


def test_plan(gpm):
    """The plan is a function of its arguments, its units cover every (target, candidate) pair exactly once, a search of
    few targets over many candidates is cut, and the workspace stays within the documented bound."""
    for N in NS:
        for m in MS:
            for targets in (N, 1, 70):
                tile, slabs, ws = gpm.vecchia_knn_plan(targets, N, m)
                assert (tile, slabs, ws) == gpm.vecchia_knn_plan(targets, N, m)
                assert tile == 64 and 1 <= slabs <= max(N, 1)
                assert (cover(targets, N, tile, slabs) == 1).all(), (targets, N, m)
                tiles = -(-targets // tile)
                assert ws == (tiles * tile * slabs * m * 12 if slabs > 1 else 0)
    assert gpm.vecchia_knn_plan(1, 1 << 20, 31)[1] >= 256, "one test point is not one lane's serial scan"
    assert gpm.vecchia_knn_plan(1 << 20, 1 << 20, 31)[1:] == (1, 0), "the causal search of many targets needs no split"
    for N in (1, 255, 256, 1000, 65536, (1 << 20) - 1, 1 << 20):
        for mz in list(range(1, 130)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096] + [N]:
            for m in (1, 31, 63):
                tile, slabs, ws = gpm.vecchia_knn_plan(mz, N, m)
                assert ws <= WS_PER_M * m and -(-mz // tile) * slabs < max(768, -(-mz // tile) + 1), (N, mz, m, slabs, ws)
                assert slabs == 1 or N // slabs >= 256, "a slab keeps 256 candidates"


def test_python_value_checks(gpm):
    """Refused before the library is called: no handle is needed."""
    g = object.__new__(gpm.GP)
    g.NDim = 3
    x, y = np.zeros((5, 3)), np.zeros(5)
    for m in (-1, 64):
        with pytest.raises(ValueError):
            g.VecchiaNeighbours(x, m)
        with pytest.raises(ValueError):
            g.SetVecchiaNearest(x, y, m)
    for bad in (np.ones(2), np.ones(4), np.ones((3, 1)), [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0], np.nan, 0.0):
        with pytest.raises(ValueError):
            g.VecchiaNeighbours(x, 2, bad)
        with pytest.raises(ValueError):
            g.SetVecchiaNearest(x, y, 2, bad)
        with pytest.raises(ValueError):
            g.VecchiaReneighbour(bad)
        with pytest.raises(ValueError):
            g.VecchiaProduceNearest(x, bad)
    with pytest.raises(ValueError):
        g.VecchiaNeighbours(x, 2, z=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        g.VecchiaNeighbours(np.zeros((5, 2)), 2)
    with pytest.raises(ValueError):
        g.VecchiaProduceNearest(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        g.SetVecchiaNearest(x, np.zeros(4), 2)
    with pytest.raises(ValueError):
        g.SetVecchiaNearest(x, y, 2, v=np.zeros(4))
    assert g.VecchiaNeighbours(x, 0).shape == (5, 0) and g.VecchiaNeighbours(np.zeros((0, 3)), 4).shape == (0, 4)
    with pytest.raises(ValueError):
        gpm.VecchiaModel(g).reneighbour(np.zeros(3))


def test_register_audit_of_the_new_kernels():
    """Every instance of the search is in the library and inside the audit's limits, with no allow-list entry."""
    _lib.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_audit
    ks = codeobj_audit.kernels(_lib.LIB_PATH)
    mine = [k for k in ks if "vknn_" in k["name"]]
    names = " ".join(k["name"] for k in mine)
    assert len([k for k in mine if "vknn_kernel" in k["name"]]) == 18, names  # 32 / 64 entries x ndim 1 .. 8 and beyond
    assert len([k for k in mine if "vknn_merge_kernel" in k["name"]]) == 2 and "vknn_scale_kernel" in names
    assert not any(re.search(pat, k["name"]) for k in mine for pat in codeobj_audit.SGPR_SPILL_ALLOW)
    assert codeobj_audit.violations(ks) == []
    for k in mine:
        assert not k.get("vgpr_spill_count", 0) and not k.get("agpr_count", 0) and not k.get("private_segment_fixed_size", 0)
        assert k["vgpr_count"] <= 128 and k.get("sgpr_spill_count", 0) <= codeobj_audit.SGPR_SPILL_LIMIT, k
