"""CPU side of tests/test_gram_kernels.py.
- The hooks of the kernels of gram.hip and of pgrad.hip's forecast derivatives refuse what a launch cannot honour, or the
  arrays do not cover, with GOGP_EARG BEFORE touching the device (device = -1 is enough to see it).
- The references of tests/gram_ref.py judge themselves on the cases the GPU test uses: the float64 evaluation of the same
  formulas passes the bounds the kernels are held to, and the exact mode's values are what those formulas give at
  inv_len = 0, bit for bit.
- gogp_test_pgrad_slabs (pgrad_slabs itself) against a restatement, and the scratch the product allocates for it.
- The product library exports none of the new hooks.
- The manifest: every __global__ of gram.hip and pgrad.hip is mapped to the hook that tests it in isolation."""
import ctypes
import os
import re

import numpy as np
import pytest

import gram_ref as R
from gogp_amd import _lib

EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
F64, F32, LD = np.float64, np.float32, np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_HOOKS = ("gogp_test_gram_split", "gogp_test_gram_local", "gogp_test_cross", "gogp_test_prior", "gogp_test_kmatvec",
             "gogp_test_pgrad", "gogp_test_pgrad_slabs")


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


# ---- refusals --------------------------------------------------------------------------------------------------------------
ARD = [dict(kind=0, ard=True, inv_len=[1.0, 2.0, 3.0])]
EV = [(0.1, 0.2, 0.5)]
PER = [dict(kind=4, w=1.0)]
TWO = [dict(kind=0), dict(kind=1)]


def call(gp, which, prec=64, ndim=3, terms=None, events=(), ev_axis=0, ev=None, radial1=0, n=100, npad=128, ld=None,
         wcols=64, k=1, bstride=0, x_len=None, out_len=None, mrows=128, ncols=128, nb_shift=6, grid=(0, 1, 0, 1), m=5, mpad=64,
         z_len=None, v_len=None, y="default", y_len=None, part_idx=0, nparts=1, nslab=3, part_len=None, alpha_len=None,
         wt_len=None, sigma_len=None, dmu_len=None, dsigma_len=None, inv_len_tail=0.0, null=None):
    """The hook `which` on device -1; every array is as long as the hook needs unless its length is given; null: the name
    of an array passed as NULL.  Returns the status."""
    H, dp = _lib.hooks(), gp._dp
    kp = gp.kparams(ndim, terms or [dict(kind=0, c=1.0, inv_len=1.0)], events=events, ev_axis=0)
    kp.ev_axis = ev_axis
    if inv_len_tail and ndim < 64:
        kp.inv_len[0][ndim] = inv_len_tail
    kps = None if null == "kparams" else (_lib.CKParams * max(k, 1))(*([kp] * max(k, 1)))
    ev = int(bool(events)) if ev is None else ev
    dt = F64 if prec == 64 else F32

    def arr(name, length, dtype=F64):
        a = np.zeros(max(int(length), 1), dtype)
        return (None, 0) if null == name else (a, int(length))

    def ptr(a, void=False):
        return None if a is None else (a.ctypes.data if void else dp(a))

    X, xl = arr("X", x_len if x_len is not None else npad * ndim + 64)
    if which == "split":
        ld = npad if ld is None else ld
        K, kl = arr("K", out_len if out_len is not None else (k - 1) * bstride + (npad - 1) * max(ld, 1) + npad, dt)
        return H.gogp_test_gram_split(-1, prec, kps, ev, ptr(X), xl, n, npad, wcols, k, bstride, ptr(K, True), kl, ld)
    if which == "local":
        ld = ncols if ld is None else ld
        K, kl = arr("K", out_len if out_len is not None else max(mrows - 1, 0) * max(ld, 1) + ncols, dt)
        pr, Pr, pc, Pc = grid
        return H.gogp_test_gram_local(-1, prec, kps, ev, ptr(X), xl, n, npad, mrows, ncols, nb_shift, pr, Pr, pc, Pc,
                                      ptr(K, True), kl, ld)
    if which == "cross":
        ld = npad if ld is None else ld
        Z, zl = arr("Z", z_len if z_len is not None else mpad * ndim)
        K, kl = arr("K", out_len if out_len is not None else max(mpad - 1, 0) * max(ld, 1) + npad, dt)
        return H.gogp_test_cross(-1, prec, kps, ev, ptr(X), xl, n, npad, ptr(Z), zl, m, mpad, ptr(K, True), kl, ld)
    if which == "prior":
        Z, zl = arr("Z", z_len if z_len is not None else m * ndim)
        P, pl = arr("prior", out_len if out_len is not None else m)
        return H.gogp_test_prior(-1, kps, ptr(Z), zl, m, ptr(P), pl)
    if which == "kmatvec":
        v, vl = arr("v", v_len if v_len is not None else npad)
        yy, yl = (None, 0) if y is None else arr("y", y_len if y_len is not None else n)
        part, pl = arr("part", part_len if part_len is not None else nslab * npad)
        out, ol = arr("out", out_len if out_len is not None else npad)
        return H.gogp_test_kmatvec(-1, kps, radial1, ev, ptr(X), xl, n, npad, ptr(v), vl, ptr(yy), yl, part_idx, nparts, nslab,
                                   ptr(part), pl, ptr(out), ol)
    assert which == "pgrad"
    ld = npad if ld is None else ld
    md = m * ndim
    ns = max(H.gogp_test_pgrad_slabs(npad, m, None), 1)
    Z, zl = arr("Z", z_len if z_len is not None else md)
    al, all_ = arr("alpha", alpha_len if alpha_len is not None else npad)
    Wt, wl = arr("Wt", wt_len if wt_len is not None else (m - 1) * max(ld, 1) + npad)
    sg, sl = arr("sigma", sigma_len if sigma_len is not None else m)
    part, pl = arr("part", part_len if part_len is not None else 2 * ns * md)
    dmu, dl = arr("dmu", dmu_len if dmu_len is not None else md)
    dsg, dsl = arr("dsigma", dsigma_len if dsigma_len is not None else md)
    return H.gogp_test_pgrad(-1, kps, ev, ptr(X), xl, n, npad, ptr(Z), zl, m, ptr(al), all_, ptr(Wt), wl, ld, ptr(sg), sl,
                             ptr(part), pl, ptr(dmu), dl, ptr(dsg), dsl)


GRAM = ("split", "local", "cross", "kmatvec", "pgrad")
BIG = 128 * 128
REFUSED = [(w, bad) for w in GRAM for bad in (
    dict(npad=96, n=90),                                  # whole 64 x 64 tiles: npad a positive multiple of 64
    dict(npad=0), dict(n=0), dict(n=129),
    dict(x_len=128 * 3 - 1),                              # the one-radial-term paths read rows n .. npad - 1 of X unguarded
    dict(null="X"), dict(null="kparams"),
    dict(terms=ARD, events=EV),                           # no instance has events and an ARD term
    dict(terms=[dict(kind=5)]), dict(terms=[dict(kind=0, ard=True), dict(kind=1, ard=True)]),
    dict(inv_len_tail=1.0), dict(ev_axis=3), dict(ev=2),
)]
REFUSED += [(w, dict(x_len=128 * 3 + 63)) for w in ("split", "local", "cross", "kmatvec")]   # ... and the slack behind X
REFUSED += [(w, bad) for w in ("split", "local", "cross") for bad in (dict(prec=16), dict(null="K"))]
REFUSED += [
    ("split", dict(wcols=0)),                             # a zero-size grid
    ("split", dict(wcols=32)), ("split", dict(wcols=96)), ("split", dict(wcols=-64)),
    ("split", dict(ld=127)), ("split", dict(out_len=127 * 128 + 127)),   # all npad rows: whole tiles are written
    ("split", dict(k=0)), ("split", dict(k=17, bstride=BIG)), ("split", dict(k=2)), ("split", dict(k=2, bstride=BIG - 64)),
    ("split", dict(k=2, bstride=BIG + 1)), ("split", dict(k=2, bstride=BIG, prec=32)),
    ("split", dict(k=2, bstride=BIG, out_len=2 * BIG - 1)),
    ("local", dict(mrows=96)), ("local", dict(ncols=0)), ("local", dict(mrows=0)), ("local", dict(ld=64)),
    ("local", dict(grid=(2, 2, 0, 1))), ("local", dict(grid=(0, 1, 0, 0))), ("local", dict(nb_shift=5)),
    ("local", dict(grid=(1, 2, 0, 1))),                   # the rank's last row lies beyond npad
    ("local", dict(out_len=127 * 128 + 127)),
    ("cross", dict(mpad=96, m=90)), ("cross", dict(mpad=0)), ("cross", dict(m=0)), ("cross", dict(m=65)),
    ("cross", dict(ld=127)), ("cross", dict(out_len=63 * 128 + 127)),    # all mpad rows
    ("cross", dict(z_len=64 * 3 - 1)), ("cross", dict(null="Z")),
    ("prior", dict(m=0)), ("prior", dict(z_len=14)), ("prior", dict(out_len=4)), ("prior", dict(null="Z")),
    ("prior", dict(null="prior")), ("prior", dict(null="kparams")), ("prior", dict(terms=[dict(kind=5)])),
    ("kmatvec", dict(radial1=1, terms=TWO)), ("kmatvec", dict(radial1=1, terms=PER)),   # radial1: one radial term
    ("kmatvec", dict(radial1=2)),
    ("kmatvec", dict(nslab=0)), ("kmatvec", dict(nslab=65)), ("kmatvec", dict(nparts=2)),  # launch_residual takes every column
    ("kmatvec", dict(y=None, nparts=0)), ("kmatvec", dict(y=None, nparts=2, part_idx=2)),
    ("kmatvec", dict(y=None, part_idx=-1)), ("kmatvec", dict(y_len=99)), ("kmatvec", dict(v_len=127)),
    ("kmatvec", dict(part_len=3 * 128 - 1)), ("kmatvec", dict(out_len=127)), ("kmatvec", dict(null="v")),
    ("kmatvec", dict(null="part")), ("kmatvec", dict(null="out")),
    ("pgrad", dict(m=0)), ("pgrad", dict(ld=127)), ("pgrad", dict(z_len=14)), ("pgrad", dict(alpha_len=127)),
    ("pgrad", dict(wt_len=4 * 128 + 127)), ("pgrad", dict(sigma_len=4)), ("pgrad", dict(part_len=2 * 2 * 15 - 1)),
    ("pgrad", dict(dmu_len=14)), ("pgrad", dict(dsigma_len=14)), ("pgrad", dict(null="Z")), ("pgrad", dict(null="alpha")),
    ("pgrad", dict(null="Wt")), ("pgrad", dict(null="sigma")), ("pgrad", dict(null="part")), ("pgrad", dict(null="dmu")),
    ("pgrad", dict(null="dsigma")),
]


def _id(wb):
    return "%s:%s" % (wb[0], ",".join("%s=%s" % (k, v if k != "terms" else len(v)) for k, v in sorted(wb[1].items())[:3]))


@pytest.mark.parametrize("which,bad", REFUSED, ids=[_id(r) for r in REFUSED])
def test_gram_hooks_refuse(gpm, which, bad):
    assert call(gpm, which, **bad) == EARG


def test_gram_hooks_accept_the_valid_neighbours(gpm):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for which in GRAM + ("prior",):
        assert call(gpm, which) in OKS, which
    for which, ok in [("split", dict(prec=32)), ("split", dict(wcols=128)), ("split", dict(wcols=256)),  # clipped to npad
                      ("split", dict(ld=136, out_len=127 * 136 + 128)), ("split", dict(n=128)),
                      ("split", dict(k=2, bstride=BIG)), ("split", dict(k=3, bstride=BIG + 2, events=EV, ev_axis=2)),
                      ("split", dict(terms=ARD)), ("split", dict(terms=TWO, events=EV)), ("split", dict(ndim=64, x_len=128 * 64 + 64)),
                      ("local", dict(prec=32)), ("local", dict(grid=(1, 2, 0, 1), npad=256, n=200)),
                      ("local", dict(nb_shift=7, mrows=128, ncols=256, grid=(1, 2, 0, 1), npad=256, out_len=127 * 256 + 256)),
                      ("local", dict(events=EV)), ("cross", dict(prec=32)), ("cross", dict(m=64)), ("cross", dict(mpad=128, m=65)),
                      ("cross", dict(events=EV, ev_axis=1)), ("prior", dict(terms=ARD)), ("prior", dict(terms=PER)),
                      ("kmatvec", dict(radial1=1)), ("kmatvec", dict(radial1=0, terms=TWO)),
                      ("kmatvec", dict(radial1=1, terms=ARD)), ("kmatvec", dict(radial1=1, events=EV)),
                      ("kmatvec", dict(y=None, nparts=3, part_idx=2)), ("kmatvec", dict(y=None)), ("kmatvec", dict(nslab=64, part_len=64 * 128)),
                      ("pgrad", dict(events=EV)), ("pgrad", dict(terms=ARD)), ("pgrad", dict(ld=136, wt_len=4 * 136 + 128)),
                      ("pgrad", dict(x_len=128 * 3)),  # its reads of X are guarded: no slack
                      ("pgrad", dict(ndim=64, m=33))]:
        assert call(gpm, which, **ok) in OKS, (which, ok)


def test_wrappers_check_types_before_the_hook(gpm):
    kp = gpm.kparams(1, [dict(kind=0)])
    z = np.zeros
    with pytest.raises(TypeError):
        gpm.gram_split_check(kp, z(128, F32), 64, 64, 64, z(64 * 64), 64)
    with pytest.raises(TypeError):
        gpm.cross_check(kp, z(128), 64, 64, z(64), 1, 64, z(64 * 64, np.int32), 64)
    with pytest.raises(gpm.GogpError):
        gpm.gram_split_check(kp, z(10), 64, 64, 64, z(64 * 64), 64)
    with pytest.raises(gpm.GogpError):
        gpm.pgrad_slabs(100, 1)


def test_the_product_library_exports_none_of_the_new_hooks(gpm):
    declared = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_HOOKS:
        assert name in declared and hasattr(_lib.hooks(), name)
        assert not hasattr(raw, name), name


# ---- pgrad_slabs -----------------------------------------------------------------------------------------------------------
def test_pgrad_slabs_against_its_restatement(gpm):
    ms = list(range(1, 200)) + [255, 256, 257, 1023, 1024, 1025, 4093, 4095, 4096, 4097, 5000]
    for tiles in (1, 2, 3, 5, 8, 16, 33, 64, 100, 255, 256, 1000, 2047, 2048):
        npad = 64 * tiles
        for m in ms:
            nslab, tps = gpm.pgrad_slabs(npad, m)
            assert (nslab, tps) == R.pgrad_slabs(npad, m), (npad, m)
            # every tile belongs to a slab, no slab is empty, and the grid of (ceil(m / 4), slabs) workgroups stays small
            assert (nslab - 1) * tps < tiles <= nslab * tps and 1 <= nslab <= max(1, 1024 // -(-m // 4)), (npad, m)
    for npad, m in [(0, 1), (100, 1), (64, 0), ((1 << 17) + 64, 1)]:
        with pytest.raises(gpm.GogpError):
            gpm.pgrad_slabs(npad, m)
    # the scratch the product hands launch_pgrad (api.hip) covers what the kernels index: part[which][slab][j][d], which < 2,
    # slab < pgrad_slabs(npad, m) -- 2 nslab m D doubles, followed there by dmu and dsigma (m D each)
    api = open(os.path.join(ROOT, "gogp_amd", "csrc", "api.hip")).read()
    assert re.search(r"nslab = gogp::pgrad_slabs\(h->npad, m, nullptr\);\s*const size_t md = \(size_t\)m \* D;\s*"
                     r"rc = h->pg_ws\.reserve\(h, md \* \(2 \* \(size_t\)nslab \+ 2\) \* sizeof\(double\)\);", api)
    assert re.search(r"\*ddmu = part \+ 2 \* \(size_t\)nslab \* md, \*ddsig = ddmu \+ md;", api)
    pg = open(os.path.join(ROOT, "gogp_amd", "csrc", "pgrad.hip")).read()
    assert "part[(((long)which * nslab + blockIdx.y) * m + jj) * D + d0 + d] = v;" in pg
    assert "const int nslab = pgrad_slabs(npad, m, &tps);" in pg and "(unsigned)nslab);" in pg


# ---- the launchers announce their dynamic LDS ----------------------------------------------------------------------------------
def test_lds_beyond_64k_is_announced():
    """With events the Gram launchers ask for 1024 D + 1024 bytes (66560 at D = 64), the matrix-vector kernels for
    (128 D + 320) 8 (+ 512 with events: 66048 from D = 62 on): every such launch site raises the function attribute."""
    assert 1024 * 64 + 1024 > 65536 >= 1024 * 63 + 1024 and (128 * 62 + 320) * 8 > 65536 >= (128 * 61 + 320) * 8 + 512
    src = open(os.path.join(ROOT, "gogp_amd", "csrc", "gram.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    for fn in ("launch_residual", "launch_kmatvec_share", "gram_lower_split_t", "gram_local_t", "cross_t"):
        body = src[src.index("void %s(" % fn):]
        body = body[:body.index("\n}\n")]
        assert "allow_lds(" in body and body.index("allow_lds(") < body.index("GOGP_KLAUNCH"), fn
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src
    assert "launch_gram_lower(" not in src and "launch_gram_lower(" not in open(
        os.path.join(ROOT, "gogp_amd", "csrc", "common.h")).read()


# ---- the references judge themselves -------------------------------------------------------------------------------------------
def within(got, want, bound, what):
    err = np.abs(np.asarray(got).astype(LD) - want).astype(F64)
    assert np.isfinite(np.asarray(got, F64)).all() and (err <= bound).all(), "%s: worst |err| / bound = %g" % (
        what, float((err[bound > 0] / bound[bound > 0]).max()))
    assert bound.max() <= 1e-10 * float(np.abs(want).max()) or np.asarray(got).dtype == F32, what + ": a loose bound"


@pytest.mark.parametrize("case", R.LD_CASES, ids=R.case_id)
def test_gram_references(case):
    sh = R.LD_SHAPE
    npad, n, m, mpad = sh["npad"], sh["n"], sh["m"], sh["mpad"]
    kp = R.kp_of(case)
    p = R.problem(case[1], npad, n, m, mpad, case[3] if case[2] else -1)
    if case[2]:  # some coordinates lie exactly on a `from` and on a `to`, and the events discount a good share of the pairs
        xa = p["x"][:, kp.ev_axis]
        assert any((xa == e[0]).any() for e in kp.events) and any((xa == e[1]).any() for e in kp.events)
        assert (R.discount(kp.events, xa, xa) != 1).mean() > 0.1
    G, E = R.padded_gram(kp, p["x"], n, npad)
    g64, _ = R.padded_gram(kp, p["x"], n, npad, "f64")
    within(g64, G, E, "gram")
    within(g64.astype(F32), G, R.padded_gram(kp, p["x"], n, npad, out32=True)[1], "gram, float")
    assert np.array_equal(G[n:], np.eye(npad)[n:]) and np.array_equal(G[:, n:], np.eye(npad)[:, n:]) and not E[n:].any()
    C, EC = R.padded_cross(kp, p["x"], n, npad, p["z"], m, mpad)
    within(R.padded_cross(kp, p["x"], n, npad, p["z"], m, mpad, "f64")[0], C, EC, "cross")
    assert not C[m:].any() and not C[:, n:].any()
    t0, t1 = R.share_tiles(npad, 1, 2)
    for y, cols in ((p["y"], None), (None, np.arange(t0 * 64, min(t1 * 64, n)))):
        want, e = R.matvec(kp, p["x"], n, p["v"], y, cols)
        within(R.matvec(kp, p["x"], n, p["v"], y, cols, "f64")[0], want, e, "matvec")


@pytest.mark.parametrize("case", R.PGRAD_CASES, ids=lambda c: R.case_id(c[:4]) + "-m%d-%d/%d" % (c[4], c[6], c[5]))
def test_pgrad_references(case):
    kind, D, nev, axis, m, npad, n = case
    kp = R.kp_of(case[:4])
    ld = npad + 8
    p = R.pgrad_problem(D, npad, n, m, ld, axis if nev else -1)
    args = (kp, p["x"], n, p["z"], m, p["alpha"], p["Wt"].reshape(m, ld), p["sigma"])
    a, ea, b, eb = R.pgrad_sums(*args)
    a64, _, b64, _ = R.pgrad_sums(*args, mode="f64")
    within(a64, a, ea, "dmu")
    within(b64, b, eb, "dsigma")


def test_the_case_tables_cover_what_they_must():
    D = {c[1] for c in R.LD_CASES}
    assert D == set(R.LD_DIMS) and {c[0] for c in R.LD_CASES} >= set(R.RADIAL) | {"periodic", "max_terms", "hyperpriors", "ard"}
    assert {c[1] for c in R.LD_CASES if c[0] == "ard"} == {5, 64}
    ev = [c for c in R.LD_CASES if c[2]]
    assert {c[2] for c in ev} >= {1, 3, R.MAX_EVENTS} and any(c[3] != 0 for c in ev)
    assert {c[1] for c in ev} >= {62, 64} and len(R.terms_of("max_terms", 3)) == R.MAX_TERMS
    assert {c[1] for c in R.PGRAD_CASES if not c[2]} == set(R.PGRAD_D) and {c[4] for c in R.PGRAD_CASES} == set(R.PGRAD_M)
    for D_ in R.PGRAD_D:
        assert {(c[5], c[6]) for c in R.PGRAD_CASES if c[1] == D_ and not c[2]} == set(R.PGRAD_SHAPES)
    for m in R.PGRAD_M:
        assert {(c[5], c[6]) for c in R.PGRAD_CASES if c[4] == m and not c[2]} == set(R.PGRAD_SHAPES)
    assert {c[1] for c in R.PGRAD_CASES if c[2]} == {3, 9, 17}
    assert {c[0] for c in R.PGRAD_CASES} >= {"periodic", "max_terms"}


@pytest.mark.parametrize("which", sorted(R.EXACT_KERNELS))
def test_exact_mode_is_what_the_formulas_give(which):
    D, npad, n = 3, 128, 100
    for ev in (False, True):
        kp, p = R.exact_kp(which, D, ev, 1), R.problem(D, npad, n, ev_axis=1)
        G = R.exact_gram(kp, p["x"], n, npad)
        for mode in ("ld", "f64"):
            g, _ = R.padded_gram(kp, p["x"], n, npad, mode)
            assert np.array_equal(g.astype(F64), G) and np.array_equal(g, G.astype(g.dtype))
        assert np.array_equal(G.astype(F32).astype(F64), G)
        if ev:
            assert len(set(G[:n, :n][~np.eye(n, dtype=bool)].tolist())) >= 3  # several discounts, and pairs without one
    # the slabs of the matrix-vector product: every tile once, ragged last slab, empty slabs and shares
    assert R.slab_columns(320, 3, 0, 5, False) == [(0, 2), (2, 4), (4, 5)]
    assert R.slab_columns(320, 8, 0, 5, False)[4:] == [(4, 5), (5, 5), (5, 5), (5, 5)]
    assert [R.share_tiles(320, i, 3) for i in range(3)] == [(0, 2), (2, 4), (4, 5)]
    assert [R.share_tiles(128, i, 3) for i in range(3)] == [(0, 1), (1, 2), (2, 2)]
    assert R.slab_columns(128, 3, 2, 2, True) == [(2, 2)] * 3 and R.slab_columns(320, 3, 2, 4, True) == [(2, 3), (3, 4), (4, 4)]


# ---- the manifest ----------------------------------------------------------------------------------------------------------------
#: kernel -> the hook (gogp_test_<name>) that drives it through its product launcher
KERNEL_HOOKS = {
    # gram.hip (each GOGP_EVN(name) is compiled twice: name and name_ev)
    "gram_kernel": "gram_split", "gram_kernel_ev": "gram_split",  # <true, T>: cross
    "gram_local_kernel": "gram_local", "gram_local_kernel_ev": "gram_local",
    "kmatvec_kernel": "kmatvec", "kmatvec_kernel_ev": "kmatvec", "kmatvec_finish_kernel": "kmatvec",
    "prior_kernel": "prior",
    # pgrad.hip
    "bwd_panel_kernel": "bwd_panel", "pgrad_kernel": "pgrad", "pgrad_kernel_ev": "pgrad", "pgrad_final_kernel": "pgrad",
}
#: the tests that drive each hook: a kernel counts as tested in isolation only if its hook is called there
HOOK_TESTS = ("test_gram_kernels.py", "test_update_kernels.py")
KERNEL_RE = r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(?:GOGP_EVN\((\w+)\)|(\w+))\s*\("


def kernels_of(src):
    src = re.sub(r"//[^\n]*", "", src)
    out = []
    for evn, plain in re.findall(KERNEL_RE, src):
        out += [evn, evn + "_ev"] if evn else [plain]
    return out


def test_every_kernel_of_the_two_files_is_tested_in_isolation():
    found = []
    for name in ("gram.hip", "pgrad.hip"):
        found += kernels_of(open(os.path.join(ROOT, "gogp_amd", "csrc", name)).read())
    assert len(found) == len(set(found)) == 12, found
    assert set(found) == set(KERNEL_HOOKS), (set(found) ^ set(KERNEL_HOOKS))
    declared = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    tests = "".join(open(os.path.join(ROOT, "tests", t)).read() for t in HOOK_TESTS)
    for kernel, hook in KERNEL_HOOKS.items():
        assert "gogp_test_" + hook in declared, (kernel, hook)
        assert hook + "_check(" in tests, "no test calls the hook of %s" % kernel
    assert "cross_check(" in tests  # gram_kernel<true, T>
    # the scan sees a templated kernel, a plain one and the GOGP_EVN(name) spelling
    probe = ("template <class T>\n__global__ __launch_bounds__(256) void new_kernel(T *p) {}\n__global__ void other_kernel() {}\n"
             "__global__ __launch_bounds__(256) void GOGP_EVN(twice_kernel)(int a) {}  // __global__ void gone_kernel()\n")
    assert kernels_of(probe) == ["new_kernel", "other_kernel", "twice_kernel", "twice_kernel_ev"]
