"""The iterative exact GP (gogp_cg_*), the part that needs no GPU: the numpy reference of tests/cg_ref.py held to the
conditions the GPU tests (tests/test_cg_gpu.py) hold the device to, the float64 evaluation of the product's reference
inside its own bound, the binding tables, and the refusals of the C calls, the hooks and the Python layer, which
validate before they touch a device.

Conditions on the reference, with alpha* from numpy.linalg.solve and cond from numpy.linalg.cond (tests/cg_ref.py: problem):
  1  tol = 1e-8: converged and rel_residual <= 2 tol (the drift between recurrence and true residual is about
     u * iterations * cond ~ 1e-9);
  2  rel_residual equals the residual recomputed in long double within the product's bound divided by |y|;
  3  |alpha - alpha*| <= (cond rel_residual + cond n u) |alpha*|;
  4  the tabulated cases: iterations at rank 64 at most those at rank 0 divided by 3.9; rank 128 on the first case with
     piv_tol = 0 stops below 128 columns;
  8  max_iter = 2 on the Matern cases: not converged, rel_residual > tol, outputs written.

Reference counterpart: none."""
import ctypes
import os
import re

import numpy as np
import pytest

import cg_ref as C
import gram_ref as R
from gogp_amd import _lib

EARG, EHIP, OK = _lib.GOGP_EARG, _lib.GOGP_EHIP, _lib.GOGP_OK
TOL = 1e-8


@pytest.mark.parametrize("name", list(C.CASES))
def test_reference_meets_the_conditions(name):
    p = C.problem(name)
    res, used = C.reference_solve(name, 64, TOL)
    a, rel = res["X"][0], float(res["rel_residual"][0])
    assert used == 64 and res["converged"][0] and rel <= 2 * TOL                                          # 1
    ld, bnd = C.true_residual_ld(p, a)
    print("%s: cond %.3g, %d iterations, rel_residual %.3g (recurrence %.3g), long double %.3g +- %.3g, |alpha - alpha*| "
          "/ bound %.3g" % (name, p["cond"], res["iterations"][0], rel, res["rel_residual_recurrence"][0], ld, bnd,
                            np.linalg.norm(a - p["alpha"]) / C.alpha_bound(p, rel)))
    assert abs(rel - ld) <= bnd                                                                           # 2
    assert np.linalg.norm(a - p["alpha"]) <= C.alpha_bound(p, rel)                                        # 3


@pytest.mark.parametrize("name", C.TABULATED)
def test_reference_preconditioner_pays(name):
    r0, _ = C.reference_solve(name, 0, TOL)
    r64, _ = C.reference_solve(name, 64, TOL)
    assert r0["converged"][0] and 3.9 * r64["iterations"][0] <= r0["iterations"][0]                       # 4


def test_reference_rank_stops_early():
    _, used = C.reference_solve(C.TABULATED[0], 128, TOL)
    assert 64 < used < 128


@pytest.mark.parametrize("name", C.MATERN)
def test_reference_max_iter(name):
    res, _ = C.reference_solve(name, 64, TOL, max_iter=2)
    assert not res["converged"][0] and res["iterations"][0] == 2 and res["rel_residual"][0] > TOL         # 8
    assert np.isfinite(res["X"]).all() and np.abs(res["X"]).max() > 0


def test_reference_columns_freeze_one_by_one():
    """A block of 17 columns, one of them zero: condition 3 per column, zeros after 0 iterations, and the columns freeze
    at different iterations."""
    p = C.problem("matern52_2d")
    rng = np.random.default_rng(5)
    B = rng.standard_normal((17, p["N"]))
    B[3] = 0.0
    B[5] *= 1e-3
    P, _ = C.precond_of(p["K"], p["d"], 64, 0.0)
    res = C.cg_block(p["Kh"], B, P, TOL, 1000)
    assert res["converged"].all() and res["iterations"][3] == 0 and not res["X"][3].any()
    assert len(set(res["iterations"].tolist())) > 2
    S = np.linalg.solve(p["Kh"], B.T).T
    for t in range(17):
        bound = (p["cond"] * res["rel_residual"][t] + p["cond"] * p["N"] * C.U) * np.linalg.norm(S[t])
        assert np.linalg.norm(res["X"][t] - S[t]) <= bound
    # (numpy's products take other paths for one row than for 17: the bit-identity of a column alone and inside a block
    # is the device's property, asserted in tests/test_cg_gpu.py, not the reference's)


def test_reference_refuses_an_indefinite_matrix():
    p = C.problem("normal_1d")
    P, _ = C.precond_of(p["K"], p["d"], 0, 0.0)
    with pytest.raises(C.NotPositiveDefinite):
        C.cg_block(-p["Kh"], p["y"][None, :], P, TOL, 10)


LD_CASES = [c for c in R.LD_CASES if c[1] in (1, 3, 8, 17, 64) and c[2] == 0]


@pytest.mark.parametrize("case", LD_CASES[::3], ids=[R.case_id(c) for c in LD_CASES[::3]])
def test_float64_product_inside_its_bound(case):
    """The plain float64 evaluation of the product's formulas against the long-double one: inside the bound the GPU test
    holds the kernel to, and the bound is tight enough to judge by."""
    kp, D = R.kp_of(case), case[1]
    rng = np.random.default_rng([95, D])
    A, V = rng.uniform(-1, 1, (97, D)), rng.standard_normal((5, 97))
    diag = rng.integers(1, 6, 97).astype(float)
    want, bound = C.kmm(kp, A, A, V, diag)
    got, _ = C.kmm(kp, A, A, V, diag, mode="f64")
    assert (np.abs(got.astype(np.longdouble) - want).astype(float) <= bound).all()
    assert bound.max() <= 1e-10 * float(np.abs(want).max())


def test_slab_model():
    assert C.slab_columns(257, 3) == [(0, 128), (128, 256), (256, 257)]
    assert C.slab_columns(100, 8) == [(0, 64), (64, 100)] + [(100, 100)] * 6
    assert C.kmm_slabs(600, 600) == 10 and C.kmm_slabs(1048576, 1048576) == 1 and C.kmm_slabs(16384, 16384) == 8


# ---- bindings ------------------------------------------------------------------------------------------------------------------
def test_symbols_bound_and_declared():
    """Fails on the parent commit: the gogp_cg_* symbols and the hooks are in the binding's tables with the headers'
    argument counts, the headers declare them and the libraries export them."""
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    hooks = {name: (res, args) for name, res, args in _lib.HOOK_SYMBOLS}
    want = {"gogp_cg_set_data": 5, "gogp_cg_solve": 9, "gogp_cg_get_alpha": 3, "gogp_cg_solve_columns": 7,
            "gogp_cg_produce": 8, "gogp_cg_last_info": 2}
    want_hooks = {"gogp_test_kmm": 21, "gogp_test_cg_dots": 19, "gogp_test_cg_update_xr": 16, "gogp_test_cg_update_p": 12,
                  "gogp_test_cg_scale": 12, "gogp_test_cg_status": 4, "gogp_test_cg_precond": 18, "gogp_test_kmm_slabs": 2,
                  "gogp_test_cg_dot_blocks": 1}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def header(name):
        with open(os.path.join(root, "include", name)) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)

    h, hh = header("gogp_hip.h"), header("gogp_testhooks.h")
    for tab, text, names in ((table, h, want), (hooks, hh, want_hooks)):
        for name, nargs in names.items():
            assert name in tab and len(tab[name][1]) == nargs, name
            m = re.search(r"int %s\(([^)]*)\);" % name, text)
            assert m and len(m.group(1).split(",")) == nargs, name
    assert ctypes.sizeof(_lib.CCgCol) == 24 and ctypes.sizeof(_lib.CCgInfo) == 24
    assert "#define GOGP_CG_MAX_RANK 1024" in h and "#define GOGP_CG_MAX_RHS  64" in h.replace("RHS 64", "RHS  64")
    _lib.build()
    lib, hk = _lib.lib(), _lib.hooks()
    for name in want:
        assert getattr(lib, name) is not None
    for name in want_hooks:
        assert getattr(hk, name) is not None
    from gogp_amd import gp
    for name in ("SetCG", "CGSolve", "CGAlpha", "CGSolveColumns", "CGProduce"):
        assert callable(getattr(gp.GP, name))
    for name in ("kmm_check", "cg_dots_check", "cg_update_xr_check", "cg_update_p_check", "cg_scale_check", "cg_status_check",
                 "cg_precond_check"):
        assert callable(getattr(gp, name))
    src = open(os.path.join(root, "gogp_amd", "host", "gogp.hpp")).read()
    for name in want:
        assert name + "(" in src, name


def test_c_abi_refuses_a_null_handle():
    _lib.build()
    L = _lib.lib()
    one = np.zeros(1)
    dp = one.ctypes.data_as(_lib._dp)
    info, col = _lib.CCgInfo(), (_lib.CCgCol * 1)()
    assert L.gogp_cg_set_data(None, dp, dp, None, 1) == EARG
    assert L.gogp_cg_solve(None, dp, 1, 0, -1.0, 1e-8, 10, ctypes.byref(info), col) == EARG
    assert L.gogp_cg_get_alpha(None, dp, 1) == EARG
    assert L.gogp_cg_solve_columns(None, dp, 1, 1e-8, 10, dp, col) == EARG
    assert L.gogp_cg_produce(None, dp, 1, dp, dp, 1e-8, 10, col) == EARG
    assert L.gogp_cg_last_info(None, ctypes.byref(info)) == EARG


# ---- the hooks refuse bad arguments before they touch a device (device = -1) ----------------------------------------------
@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _kmm(gp, **a):
    g = lambda k, d: a.get(k, d)  # noqa: E731
    D, rows, cols, T, nslab = 2, g("rows", 100), g("cols", 70), g("T", 3), g("nslab", 2)
    kp = gp.kparams(D, [dict(kind=g("kind", 0), c=1.5, inv_len=0.7)], events=g("events", ()))
    A, B = np.zeros(g("a_len", 100 * D)), np.zeros(g("b_len", 70 * D))
    ldv = g("ldv", 72)
    V = np.zeros(g("v_len", 2 * 72 + 70))
    diag = np.zeros(g("diag_len", 100)) if g("with_diag", False) else None
    part, out = np.zeros(g("part_len", 2 * 3 * 128)), np.zeros(g("out_len", 3 * 101))
    return gp.kmm_check(kp, A, rows, None if g("square", False) else B, cols, V, ldv, T, diag, nslab, part, out, g("ldo", 101),
                        max_blocks=g("max_blocks", 0))


KMM_REFUSED = [dict(rows=0), dict(cols=0), dict(rows=(1 << 15) + 1), dict(T=0), dict(T=65), dict(nslab=0), dict(nslab=65),
               dict(max_blocks=-1), dict(a_len=199), dict(b_len=139), dict(ldv=69), dict(v_len=2 * 72 + 69),
               dict(part_len=2 * 3 * 128 - 1), dict(out_len=3 * 101 - 1), dict(ldo=99), dict(square=True),
               dict(with_diag=True), dict(square=True, cols=100, v_len=2 * 102 + 100, ldv=102, with_diag=True, diag_len=99),
               dict(kind=7), dict(events=((0.0, 1.0, 0.5),))]


@pytest.mark.parametrize("bad", KMM_REFUSED, ids=[",".join("%s=%s" % kv for kv in d.items()) for d in KMM_REFUSED])
def test_kmm_hook_refuses(gpm, bad):
    with pytest.raises(gpm.GogpError) as e:
        _kmm(gpm, **bad)
    assert e.value.code == EARG


def test_hooks_pass_good_arguments_on_to_the_device(gpm):
    """A well-formed call gets as far as the device: without a GPU it comes back GOGP_EHIP, never GOGP_EARG; with one it
    returns the arrays."""
    for kw in (dict(), dict(square=True, cols=100, v_len=2 * 102 + 100, ldv=102, with_diag=True)):
        try:
            part, out = _kmm(gpm, **kw)
        except gpm.GogpError as e:
            assert e.code == EHIP, kw
        else:
            assert part.shape == (2 * 3 * 128,) and out.shape == (3 * 101,), kw


def _vec_calls(gp, n=10, T=2, ld=12, short=0, sc_len=6 * 64, st_len=4 * 64, mode="pq", nblk=None):
    size = (max(T, 1) - 1) * ld + max(n, 1)
    blk, full = np.zeros(size - short), np.zeros(size)
    sc, st = np.zeros(sc_len), np.zeros(st_len, dtype=np.int32)
    part = np.zeros(max(T, 1) if nblk is None else nblk)
    return [lambda: gp.cg_dots_check(blk, full, ld, n, T, mode, 1, 1e-8, part, np.zeros(max(T, 1)), sc, st),
            lambda: gp.cg_update_xr_check(full, full, blk, full, ld, n, T, sc, st),
            lambda: gp.cg_update_p_check(full, blk, ld, n, T, sc, st),
            lambda: gp.cg_scale_check(blk, None, None, ld, n, T, full) if short else
            gp.cg_scale_check(full, np.zeros(max(n - 1, 1)), None, ld, max(n, 2), T, full),
            lambda: gp.cg_precond_check(None, ld, n, 0, np.zeros(max(n, 1)), None, blk, ld, T, full) if short else
            gp.cg_precond_check(np.zeros(max(n, 1)), ld, n, 0, np.zeros(max(n, 1)), None, full, ld, T, full)]


@pytest.mark.parametrize("bad", [dict(short=1), dict(n=0), dict(T=0), dict(T=65), dict(ld=9), dict(sc_len=6 * 64 - 1),
                                 dict(st_len=4 * 64 - 1)], ids=str)
def test_vector_hooks_refuse(gpm, bad):
    calls = _vec_calls(gpm, **bad)
    if "sc_len" in bad or "st_len" in bad:
        calls = calls[:3]
    for call in calls:
        with pytest.raises(gpm.GogpError) as e:
            call()
        assert e.value.code == EARG


def test_more_refusals(gpm):
    full, sc, st = np.zeros(22), np.zeros(6 * 64), np.zeros(4 * 64, dtype=np.int32)
    for call in (lambda: gpm.cg_dots_check(full, full, 12, 10, 2, 6, 1, 1e-8, np.zeros(2), np.zeros(2), sc, st),
                 lambda: gpm.cg_dots_check(full, full, 12, 10, 2, "plain", 1, 1e-8, np.zeros(2), None, sc, st),
                 lambda: gpm.cg_dots_check(full, full, 12, 10, 2, "pq", 1, 1e-8, np.zeros(1), None, sc, st),
                 lambda: gpm.cg_status_check(0, st), lambda: gpm.cg_status_check(65, st),
                 lambda: gpm.cg_status_check(1, st[:-1].copy()),
                 lambda: gpm.cg_precond_check(np.zeros(3 * 12), 12, 10, 3, np.zeros(10), np.zeros(255), full, 12, 2, full),
                 lambda: gpm.cg_precond_check(np.zeros(3 * 12 - 3), 12, 10, 3, np.zeros(10), np.zeros(256), full, 12, 2, full),
                 lambda: gpm.cg_precond_check(np.zeros(3 * 12), 12, 10, 1025, np.zeros(10), np.zeros(256), full, 12, 2, full)):
        with pytest.raises(gpm.GogpError) as e:
            call()
        assert e.value.code == EARG
    assert gpm.kmm_slabs(600, 600) == 10 and gpm.cg_dot_blocks(2049) == 2
    with pytest.raises(gpm.GogpError):
        gpm.kmm_slabs(0, 1)
    # the Python layer's own checks
    with pytest.raises(TypeError):
        gpm.cg_status_check(1, np.zeros(256))  # not int32
    with pytest.raises(TypeError):
        gpm.cg_scale_check(np.zeros((4, 4))[:, :2], None, None, 2, 2, 1, np.zeros(2))  # not contiguous
    with pytest.raises(TypeError):
        gpm.cg_dots_check(np.zeros(4, dtype=np.float32), np.zeros(4), 4, 4, 1, "plain", 0, 1.0, np.zeros(1), np.zeros(1), sc, st)
