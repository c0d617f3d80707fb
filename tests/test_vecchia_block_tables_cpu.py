"""Block tables built on the device (gogp_vecchia_blocks_nearest and its kin, gogp_amd/csrc/vecchia_bknn.hip), the part
that needs no GPU: the binding tables, the refusals made before a device is touched, the plan of the search, the value
checks of the Python methods, the host's centroid and the register audit of the new kernels.

Reference counterpart: none."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import vecchia_bknn_ref as R
from gogp_amd import _lib

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"gogp_vecchia_blocks_nearest": 11, "gogp_vecchia_blocks_set_data_nearest": 8, "gogp_vecchia_blocks_reneighbour": 2,
         "gogp_vecchia_blocks_get_table": 4, "gogp_vecchia_blocks_produce_nearest": 9}
HOOKS = {"gogp_test_vecchia_bknn": 21, "gogp_test_vecchia_bknn_plan": 4}
WS_PER_C = 768 * 8 * 12  # include/gogp_testhooks.h: the workspace stays under this many bytes per entry of a list


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def test_binding_tables(gpm):
    def header(name):
        with open(os.path.join(ROOT, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    for tab, text, names, L in ((_lib.SYMBOLS, header("gogp_hip.h"), CALLS, _lib.lib()),
                                (_lib.HOOK_SYMBOLS, header("gogp_testhooks.h"), HOOKS, _lib.hooks())):
        tab = {name: args for name, _, args in tab}
        for name, nargs in names.items():
            assert len(tab[name]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
            assert getattr(L, name) is not None
    for name in ("VecchiaBlockTables", "SetVecchiaBlocksNearest", "VecchiaBlockReneighbour", "VecchiaBlockTable",
                 "VecchiaBlockProduceNearest"):
        assert callable(getattr(gpm.GP, name)) and name not in vars(gpm.GP)
    assert callable(gpm.VecchiaBlockModel.reneighbour)
    src = open(os.path.join(ROOT, "gogp_amd", "host", "gogp.hpp")).read()
    shim = open(os.path.join(ROOT, "go", "gogp", "gp.go")).read()
    for name in CALLS:
        assert name + "(" in src and "C." + name + "(" in shim, name


def test_c_abi_refuses_a_null_handle():
    _lib.build()
    L = _lib.lib()
    one, t = np.ones(1), np.full(4, -1, np.int32)
    dp, tp = one.ctypes.data_as(_lib._dp), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.gogp_vecchia_blocks_nearest(None, dp, 1, None, 0, 1, 1, dp, tp, tp, tp) == EARG
    assert L.gogp_vecchia_blocks_set_data_nearest(None, dp, dp, None, 1, 1, 1, dp) == EARG
    assert L.gogp_vecchia_blocks_reneighbour(None, dp) == EARG
    assert L.gogp_vecchia_blocks_get_table(None, tp, tp, tp) == EARG
    assert L.gogp_vecchia_blocks_produce_nearest(None, dp, 1, 1, 1, dp, dp, None, None) == EARG


def test_hook_refuses_bad_arguments_before_the_device(gpm):
    X = np.arange(24, dtype=np.float64)

    def call(n=8, ndim=3, t=2, c=3, **kw):
        try:
            gpm.vecchia_bknn_check(X, n, ndim, t, c, **kw)
        except gpm.GogpError as e:
            return e.code
        return OK

    assert call(n=9) == EARG and call(n=0) == EARG and call(ndim=0) == EARG and call(ndim=65) == EARG
    assert call(t=0) == EARG and call(c=-1) == EARG and call(c=129) == EARG
    assert call(qt=-1) == EARG and call(qt=9) == EARG and call(slabs=-1) == EARG and call(slabs=257) == EARG
    assert call(Z=np.zeros(5), mz=2) == EARG and call(Z=np.zeros(6), mz=0) == EARG and call(mz=3) == EARG
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.inf, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0]):
        assert call(lengths=np.array(bad)) == EARG
    assert call() in (OK, EHIP), "a well-formed call gets as far as the device"
    assert call(Z=np.zeros(6), mz=2, lengths=np.ones(3), qt=3, slabs=3) in (OK, EHIP)
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, -1), (5, 5, 129)):
        with pytest.raises(gpm.GogpError):
            gpm.vecchia_bknn_plan(*bad)


def test_plan(gpm):
    """The plan is a function of its arguments, its units cover every (query, candidate) pair exactly once, a search of
    few queries over many candidates is cut, and the workspace stays within the documented bound."""
    for n in (1, 2, 63, 64, 65, 129, 257, 1000):
        for queries in (n, 1, 9, 70):
            for c in (0, 1, 64, 65, 128):
                qt, slabs, ws = gpm.vecchia_bknn_plan(queries, n, c)
                assert (qt, slabs, ws) == gpm.vecchia_bknn_plan(queries, n, c)
                assert qt == min(8, queries) and 1 <= slabs <= max(n, 1)
                hits = np.zeros((queries, n), dtype=np.int64)
                L = -(-n // slabs)
                for q0 in range(0, queries, qt):
                    for s in range(slabs):
                        hits[q0:min(queries, q0 + qt), s * L:min(n, (s + 1) * L)] += 1
                assert (hits == 1).all(), (queries, n, c)
                assert ws == (-(-queries // qt) * qt * slabs * c * 12 if slabs > 1 else 0)
    assert gpm.vecchia_bknn_plan(1, 1 << 20, 64)[1] >= 256, "one test group is not one workgroup's serial scan"
    assert gpm.vecchia_bknn_plan(1 << 14, 1 << 20, 64)[1:] == (1, 0), "the causal search of many blocks needs no split"
    for n in (1, 255, 256, 1000, 65536, (1 << 20) - 1, 1 << 20):
        for queries in list(range(1, 130)) + [255, 256, 257, 2047, 2048, 2049, 4096, n]:
            for c in (1, 64, 128):
                qt, slabs, ws = gpm.vecchia_bknn_plan(queries, n, c)
                assert ws <= WS_PER_C * c, (n, queries, c, slabs, ws)
                assert slabs == 1 or n // slabs >= 256, "a slab keeps 256 candidates"


def test_python_value_checks(gpm):
    """Refused before the library is called: no handle is needed."""
    g = object.__new__(gpm.GP)
    g.NDim = 3
    x, y = np.zeros((5, 3)), np.zeros(5)
    calls = []
    for t, c in ((0, 1), (1, -1), (1, 128), (64, 65), (129, 0)):
        calls += [lambda t=t, c=c: g.VecchiaBlockTables(x, t, c), lambda t=t, c=c: g.SetVecchiaBlocksNearest(x, y, t, c)]
    for gz, c in ((0, 1), (1, -1), (1, 129)):
        calls += [lambda gz=gz, c=c: g.VecchiaBlockTables(x, gz, c, z=x), lambda gz=gz, c=c: g.VecchiaBlockProduceNearest(x, gz, c)]
    for bad in (np.ones(2), np.ones((3, 1)), [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0], np.nan, 0.0):
        calls += [lambda b=bad: g.VecchiaBlockTables(x, 2, 2, b), lambda b=bad: g.SetVecchiaBlocksNearest(x, y, 2, 2, b),
                  lambda b=bad: g.VecchiaBlockReneighbour(b), lambda b=bad: g.VecchiaBlockProduceNearest(x, 2, 2, b)]
    calls += [lambda: g.VecchiaBlockTables(x, 2, 2, z=np.zeros((4, 2))), lambda: g.SetVecchiaBlocksNearest(x, np.zeros(4), 2, 2),
              lambda: g.SetVecchiaBlocksNearest(x, y, 2, 2, v=np.zeros(4)),
              lambda: gpm.VecchiaBlockModel(g).reneighbour(np.zeros(3))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    assert g.VecchiaBlockTables(np.zeros((0, 3)), 4, 4)[0].shape == (0, 8)


@pytest.mark.parametrize("D", [1, 2, 3, 9])
def test_centroid_is_the_row_order_sum(D):
    """vecchia._centroid against the explicit sum, D = 1 with 8 or more rows included, where ndarray.mean differs."""
    from gogp_amd import vecchia as VT
    for n, t in ((1, 1), (7, 3), (64, 8), (130, 128), (1000, 9), (1000, 16), (1000, 128)):
        xs = R.rows(n, D, "random") * 1e3
        got, want = VT._centroid(xs, t), R.centroids(xs, t)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, t, D)
    x = R.rows(200, D, "grid")
    tbl, nc, nt = VT.block_nearest(x, 16, 20)
    assert [np.array_equal(a, b) for a, b in zip((tbl, nc, nt), R.pack(*R.causal(x, 16, 20)[::2], 200, 16))] == [True] * 3


def test_register_audit_of_the_new_kernels():
    """Every instance of the new kernels is in the library and inside the audit's limits, with no allow-list entry."""
    _lib.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_audit
    ks = codeobj_audit.kernels(_lib.LIB_PATH)
    mine = [k for k in ks if "bknn_" in k["name"]]
    names = " ".join(k["name"] for k in mine)
    assert len([k for k in mine if "bknn_select_kernel" in k["name"]]) == 18, names  # 64 / 128 entries x ndim 1 .. 8 and beyond
    assert len([k for k in mine if "bknn_merge_kernel" in k["name"]]) == 2
    assert "bknn_centroid_kernel" in names and "bknn_pack_kernel" in names
    assert not any(re.search(pat, k["name"]) for k in mine for pat in codeobj_audit.SGPR_SPILL_ALLOW)
    assert codeobj_audit.violations(ks) == []
    for k in mine:
        assert not k.get("vgpr_spill_count", 0) and not k.get("agpr_count", 0) and not k.get("private_segment_fixed_size", 0)
        assert k["vgpr_count"] <= 256 and k.get("sgpr_spill_count", 0) <= codeobj_audit.SGPR_SPILL_LIMIT, k
