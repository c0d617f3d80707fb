"""CPU side of tests/test_update_kernels.py.
- The hooks of the append, remove, skinny-product and predictive-covariance kernels refuse what a launch cannot honour, or
  the arrays do not cover, with GOGP_EARG BEFORE touching the device (device = -1 is enough to see it).
- pcov_slabs over a sweep of (npad, m, ncu): whole 256-column panels, the slabs cover npad and none is empty.
- The references of tests/update_kernels_ref.py judge themselves: the integer cases are exact in float64, and float64 runs
  of the same operations pass the bounds the kernels are held to, with every bound under the cap of judge()."""
import numpy as np
import pytest

import update_kernels_ref as R
from gogp_amd import _lib
from test_substitution_kernels import judge, same_bits

EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
AP = R.APPEND_PART


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def z(n, dt=np.float64):
    return np.zeros(max(int(n), 1), dt)


def kp_of(gp, ndim=2, terms=None, ev_axis=1, inv_len_tail=0.0):
    kp = gp.kparams(ndim, terms or [dict(kind=0, c=4.0, inv_len=0.0)], events=R.EVENTS, ev_axis=0)
    kp.ev_axis = ev_axis
    if inv_len_tail:
        kp.inv_len[0][ndim] = inv_len_tail
    return kp


def call(gp, which, **a):
    """The hook `which` with valid arguments of a small launch, overridden by a; returns the status."""
    H, dp = _lib.hooks(), gp._dp
    ip = lambda v: v.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_int))  # noqa: E731
    g = lambda k, d: a.get(k, d)  # noqa: E731
    if which == "gram":
        npc, m, m0, n = g("npc", 256), g("m", 40), g("m0", 32), g("n", 250)
        ld = g("ld", 260)
        k0, w0, o0 = g("kind0", R.TS_SOL_PAIRED), g("width0", 32), g("off0", 16)
        k1, w1, o1 = g("kind1", R.TS_SOL_COMPACT), g("width1", 8), g("off1", 8)
        s0 = np.zeros(g("sol0_len", 16 + 256 * 32 * 8), np.uint8)
        s1 = np.zeros(g("sol1_len", 8 + 256 * 8 * 8), np.uint8)
        zz, part, Ln = z(g("z_len", 256)), z(g("part_len", AP)), z(g("lnew_len", 39 * 260 + 250))
        return H.gogp_test_append_gram(-1, None if g("sol0_null", False) else s0.ctypes.data, s0.size, k0, w0, o0,
                                       None if g("sol1_null", False) else s1.ctypes.data, s1.size, k1, w1, o1, m0, m, npc, n,
                                       dp(zz), zz.size, dp(part), part.size, dp(Ln), Ln.size, ld)
    if which == "commit":
        m, n, nslab, ld = g("m", 17), g("n", 300), g("nslab", 3), g("ld", 320)
        kp = kp_of(gp, terms=g("terms", None), ev_axis=g("ev_axis", 1), inv_len_tail=g("inv_len_tail", 0.0))
        X2, y2, part = z(g("x2_len", 34)), z(g("y2_len", 17)), z(g("part_len", 3 * AP))
        Ln, z2 = z(g("lnew_len", 16 * 320 + 317)), z(g("z2_len", 17))
        info = _lib.ctypes.c_longlong(0)
        return H.gogp_test_append_commit(-1, kp, g("ev", 1), dp(X2), X2.size, dp(y2), y2.size, m, n, dp(part), part.size,
                                         nslab, dp(Ln), Ln.size, ld, dp(z2), z2.size,
                                         None if g("info_null", False) else _lib.ctypes.byref(info))
    if which in ("gather", "w"):
        n1, npad1, ld0 = g("n1", 100), g("npad1", 256), g("ld0", 256)
        src = z(g("src_len", 140 * 256))
        map_ = np.arange(n1 if n1 > 0 else 1, dtype=np.int32) + g("map_shift", 40)
        map_[0] = g("map0", map_[0])
        rem = np.arange(g("rem_len", 32), dtype=np.int32)
        rem[0] = g("rem0", 0)
        if which == "gather":
            dst = z(g("dst_len", 256 * 256))
            return H.gogp_test_remove_gather(-1, dp(src), src.size, ld0, ip(map_), g("map_len", map_.size), n1, dp(dst),
                                             dst.size, npad1)
        W = z(g("w_len", 32 * 256))
        return H.gogp_test_remove_w(-1, dp(src), src.size, ld0, ip(map_), g("map_len", map_.size), ip(rem), rem.size,
                                    g("mc", 5), g("mw", 32), g("r0", 128), n1, npad1, dp(W), W.size)
    if which == "block":
        ld, mw = g("ld", 512), g("mw", 32)
        L, W, snap = z(g("l_len", 512 * 512)), z(g("w_len", 32 * 512)), z(g("snap_len", 512 * 128))
        return H.gogp_test_remove_block(-1, dp(L), L.size, ld, g("b0", 1), g("nb", 3), dp(snap), snap.size, dp(W), W.size, mw,
                                        g("kb0", 128), g("kb1", 384), g("n1", 385))
    if which == "panel":
        rows16, K, ncols = g("rows16", 3), g("K", 256), g("ncols", 128)
        lda, ldb, ldc = g("lda", 260), g("ldb", 132), g("ldc", 130)
        A, B, C = z(g("a_len", 8 + 63 * 260 + 256)), z(g("b_len", 255 * 132 + 128)), z(g("c_len", 4 + 63 * 130 + 128))
        return H.gogp_test_bwd_panel(-1, rows16, dp(A), A.size, g("a_off", 8), lda, dp(B), B.size, g("b_off", 0), ldb, dp(C),
                                     C.size, g("c_off", 4), ldc, ncols, K, g("tri", 0), g("sub", 1))
    assert which == "pcov"
    m, npad, ncu, mo, ldo, ld = g("m", 65), g("npad", 1280), g("ncu", 1), g("mo", 70), g("ldo", 72), g("ld", 1282)
    kp = kp_of(gp, terms=g("terms", None), ev_axis=g("ev_axis", 1))
    Z, Vt = z(g("z_len", 130)), z(g("vt_len", 64 * 1282 + 1280))
    part, out = z(g("part_len", 2 * 3 * 4096)), z(g("out_len", 69 * 72 + 70))
    return H.gogp_test_pcov(-1, kp, g("ev", 0), dp(Z), Z.size, m, None if g("vt_null", False) else dp(Vt), Vt.size, ld, npad,
                            ncu, None if g("part_null", False) else dp(part), part.size, 0.5, dp(out), out.size, mo, ldo)


ARD = [dict(kind=0, ard=True, inv_len=[1.0, 2.0])]
REFUSED = [
    ("gram", dict(m=0)), ("gram", dict(m=65)), ("gram", dict(m0=41)), ("gram", dict(m0=-1)),
    ("gram", dict(npc=300)), ("gram", dict(npc=0)), ("gram", dict(n=257)), ("gram", dict(n=-1)), ("gram", dict(ld=249)),
    ("gram", dict(z_len=255)), ("gram", dict(part_len=AP - 1)), ("gram", dict(lnew_len=39 * 260 + 249)),
    ("gram", dict(sol0_len=16 + 256 * 32 * 8 - 1)),        # the first source does not cover its layout
    ("gram", dict(sol1_len=8 + 256 * 8 * 8 - 1)),
    ("gram", dict(width0=16)),                             # 32 columns in a layout of 16
    ("gram", dict(width1=4)),
    ("gram", dict(kind0=R.TS_SOL_GRANULE)),                # a granule holds one right-hand side
    ("gram", dict(kind1=R.TS_SOL_GRANULE, width1=1, off1=8, m=33)),   # 16-byte loads
    ("gram", dict(kind1=4)), ("gram", dict(off0=12)), ("gram", dict(off1=-8)),
    ("gram", dict(kind0=R.TS_SOL_ROWS, width0=255)),       # ROWS: a row of the solutions is shorter than npc
    ("gram", dict(sol1_null=True)),                        # columns are read from it
    ("commit", dict(m=0)), ("commit", dict(m=65)), ("commit", dict(n=-1)), ("commit", dict(nslab=0)),
    ("commit", dict(x2_len=33)), ("commit", dict(y2_len=16)), ("commit", dict(z2_len=16)),
    ("commit", dict(part_len=3 * AP - 1)), ("commit", dict(ld=316)), ("commit", dict(lnew_len=16 * 320 + 316)),
    ("commit", dict(info_null=True)), ("commit", dict(ev_axis=2)), ("commit", dict(inv_len_tail=1.0)),
    ("commit", dict(terms=ARD, ev=1)),                     # no instance has events and ARD
    ("commit", dict(terms=[dict(kind=9)])),
    ("gather", dict(npad1=300)), ("gather", dict(n1=0)), ("gather", dict(n1=257)), ("gather", dict(map_len=99)),
    ("gather", dict(dst_len=256 * 256 - 1)), ("gather", dict(map0=-1)), ("gather", dict(map0=256)),
    ("gather", dict(src_len=139 * 256)),                   # the last mapped row is not in src
    ("w", dict(mc=0)), ("w", dict(mc=33)), ("w", dict(mw=33)), ("w", dict(mw=4, mc=5)), ("w", dict(r0=256)),
    ("w", dict(r0=-1)), ("w", dict(w_len=32 * 256 - 1)), ("w", dict(rem_len=4)), ("w", dict(rem0=256)),
    ("w", dict(map0=-3)), ("w", dict(n1=300)),
    ("block", dict(mw=8)), ("block", dict(ld=500)), ("block", dict(kb0=64)), ("block", dict(kb1=0)),
    ("block", dict(kb1=512)),                              # the block's rows of W lie beyond ldw = ld
    ("block", dict(n1=513)), ("block", dict(n1=0)), ("block", dict(b0=2, nb=3)), ("block", dict(nb=-1)),
    ("block", dict(l_len=512 * 512 - 1)), ("block", dict(w_len=32 * 512 - 1)), ("block", dict(snap_len=4 * 16384 - 1)),
    ("panel", dict(rows16=0)), ("panel", dict(ncols=96)), ("panel", dict(ncols=0)), ("panel", dict(K=48)),
    ("panel", dict(K=0)), ("panel", dict(lda=255)), ("panel", dict(ldb=127)), ("panel", dict(ldc=127)),
    ("panel", dict(a_len=8 + 47 * 260 + 256)),             # 48 rows given: beyond 32 the kernel takes groups of 64
    ("panel", dict(c_len=4 + 47 * 130 + 128)),
    ("panel", dict(b_len=255 * 132 + 127)), ("panel", dict(a_off=9)), ("panel", dict(c_off=-1)),
    ("panel", dict(rows16=5)),                             # 128 rows
    ("pcov", dict(m=0)), ("pcov", dict(mo=64)), ("pcov", dict(ldo=69)), ("pcov", dict(out_len=69 * 72 + 69)),
    ("pcov", dict(z_len=129)), ("pcov", dict(npad=1200)), ("pcov", dict(npad=0)), ("pcov", dict(ncu=0)),
    ("pcov", dict(ld=1281)),                               # 16-byte loads of the rows of Vt
    ("pcov", dict(ld=1278)), ("pcov", dict(vt_len=64 * 1282 + 1279)),
    ("pcov", dict(part_len=2 * 3 * 4096 - 1)), ("pcov", dict(part_null=True)),
    ("pcov", dict(ncu=256)),                               # five slabs: part is too short
    ("pcov", dict(ev=1, ev_axis=2)), ("pcov", dict(terms=ARD, ev=1)),
]


@pytest.mark.parametrize("which,bad", REFUSED, ids=["%s:%s" % (w, ",".join("%s=%s" % (k, v if k != "terms" else len(v))
                                                                          for k, v in d.items())) for w, d in REFUSED])
def test_update_hooks_refuse(gpm, which, bad):
    assert call(gpm, which, **bad) == EARG


def test_update_hooks_accept_the_valid_neighbours(gpm):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for which, ok in [("gram", {}), ("gram", dict(m=32, sol1_null=True)), ("gram", dict(n=0)), ("gram", dict(n=256, ld=256)),
                      ("gram", dict(kind0=R.TS_SOL_ROWS, width0=256, m=32, sol1_null=True)),
                      ("gram", dict(m=1, m0=1, kind0=R.TS_SOL_GRANULE, width0=1, lnew_len=250)),
                      ("commit", {}), ("commit", dict(ev=0)), ("commit", dict(terms=ARD, ev=0)), ("commit", dict(n=0, ld=17)),
                      ("gather", {}), ("gather", dict(n1=256, map_shift=0, src_len=256 * 256)), ("w", {}), ("w", dict(mw=4, mc=4)),
                      ("w", dict(mw=7, mc=3, r0=255)), ("block", {}), ("block", dict(mw=4)), ("block", dict(nb=0)),
                      ("block", dict(kb0=384, kb1=384, n1=512)), ("panel", {}), ("panel", dict(rows16=4)),
                      ("panel", dict(rows16=2, tri=1, sub=0)), ("pcov", {}), ("pcov", dict(vt_null=True, part_null=True)),
                      ("pcov", dict(ev=1)), ("pcov", dict(mo=65, ldo=65, out_len=65 * 65))]:
        assert call(gpm, which, **ok) in OKS, (which, ok)


def test_wrappers_check_types_before_the_hook(gpm):
    with pytest.raises(TypeError):
        gpm.remove_gather_check(z(256 * 256), 256, np.arange(100), 100, z(256 * 256), 256)  # int64 map
    with pytest.raises(TypeError):
        gpm.bwd_panel_check(1, z(16 * 32, np.float32), 0, 32, z(32 * 64), 0, 64, z(16 * 64), 0, 64, 64, 32)
    with pytest.raises(gpm.GogpError):
        gpm.bwd_panel_check(1, z(16 * 32 - 1), 0, 32, z(32 * 64), 0, 64, z(16 * 64), 0, 64, 64, 32)
    with pytest.raises(gpm.GogpError):
        gpm.pcov_slabs(100, 1, 256)


# ---- pcov_slabs -----------------------------------------------------------------------------------------------------
def test_pcov_slabs_sweep(gpm):
    seen = set()
    for npad in list(range(256, 4097, 256)) + [16384, 65536]:
        for m in (1, 17, 64, 65, 130, 512, 1000, 1024, 4096):
            for ncu in (1, 2, 8, 64, 104, 256, 304):
                nslab, cps = gpm.pcov_slabs(npad, m, ncu)
                assert (nslab, cps) == R.slabs_ref(npad, m, ncu), (npad, m, ncu)
                assert nslab >= 1 and cps % 256 == 0 and nslab * cps >= npad and (nslab - 1) * cps < npad, (npad, m, ncu)
                seen.add((nslab > 1, cps > 256, nslab * cps > npad, nslab >= 9))
    assert len(seen) >= 6  # one panel or several per slab, ragged last slabs, more than eight slabs
    for key, want in R.PCOV_SLABS.items():
        m, npad, ncu = key
        assert gpm.pcov_slabs(npad, m, ncu) == want


# ---- the references judge themselves -----------------------------------------------------------------------------------
@pytest.mark.parametrize("npc", [256, 768])
def test_gram_reference(npc):
    for m in (1, 17, 64):
        V, zz = R.gram_problem(npc, True)
        G, dots, LT, _, _ = R.gram_ref(V[:, :m], zz, npc - 3, True)
        for s in range(npc // 256):
            Vs = V[s * 256:(s + 1) * 256, :m]
            assert np.array_equal(Vs.T @ Vs, G[s, :m, :m]) and np.array_equal(Vs.T @ zz[s * 256:(s + 1) * 256], dots[s, :m])
        V, zz = R.gram_problem(npc, False)
        G, dots, LT, eG, ed = R.gram_ref(V[:, :m], zz, npc - 3, False)
        for s in range(npc // 256):
            Vs = V[s * 256:(s + 1) * 256, :m]
            judge(Vs.T @ Vs, G[s, :m, :m], eG[s, :m, :m], "V^T V")
            judge(Vs.T @ zz[s * 256:(s + 1) * 256], dots[s, :m], ed[s, :m], "V^T z")


def test_gram_sources_decode_to_V():
    import substitution_ref as S
    V, _ = R.gram_problem(256, False)
    for m in R.GRAM_M:
        (r0, k0, w0, o0), (r1, k1, w1, o1), m0 = R.gram_sources(V[:, :m])
        assert (k0, w0) == S.expected_solution(64, 0, m0)[1:] and (m <= 32 or (k1, w1) == S.expected_solution(64, 32, m - 32)[1:])
        got = S.decode_solution(r0, k0, w0, o0, 256)[:, :m0]
        if m > 32:
            got = np.hstack([got, S.decode_solution(r1, k1, w1, o1, 256)[:, :m - 32]])
        assert same_bits(np.ascontiguousarray(got), np.ascontiguousarray(V[:, :m]))


@pytest.mark.parametrize("m,nslab,n,ev", R.COMMIT_CASES)
def test_commit_reference_is_exact_in_float64(m, nslab, n, ev):
    pr = R.commit_problem(m, nslab, ev, 100 * m + nslab)
    L, z2, bad = R.commit_f64(pr, m, nslab, ev)
    assert bad is None and same_bits(L, pr["L0"]) and same_bits(z2, pr["z0"])
    assert not ev or m == 1 or len(np.unique(R.simil_exact(pr["X2"][:, 1], True))) > 1, "no pair is discounted"


@pytest.mark.parametrize("m,pivot,how", R.NOTPD_CASES)
def test_commit_reference_meets_the_bad_pivot(m, pivot, how):
    pr = R.commit_problem(m, 3, True, 7 * m + pivot, bad=(pivot, how))
    assert R.commit_f64(pr, m, 3, True)[2] == pivot


def test_panel_and_pcov_references():
    rng = np.random.default_rng(5)
    for exact in (True, False):
        A = rng.integers(-1, 2, (64, 1024)).astype(np.float64) if exact else rng.standard_normal((64, 1024))
        B = rng.integers(-1, 2, (1024, 128)).astype(np.float64) if exact else rng.standard_normal((1024, 128))
        C0 = rng.integers(-8, 9, (64, 128)).astype(np.float64) if exact else rng.standard_normal((64, 128))
        for sub in (False, True):
            want, e = R.panel_ref(A, B, C0, sub, exact)
            judge(C0 - A @ B if sub else A @ B, want, e, "panel")
    for m, npad, ncu, mo, ev in R.PCOV_CASES:
        if npad is None:
            continue
        nslab, cps = R.slabs_ref(npad, m, ncu)
        Kz = R.simil_exact(R.points(m, 600 + m)[:, 1], ev)
        for exact in (True, False):
            Vd = rng.integers(-1, 2, (m, npad)).astype(np.float64) if exact else rng.standard_normal((m, npad))
            part, out, e_part, e_out = R.pcov_ref(Vd, Kz, 0.5, nslab, cps, mo, exact)
            got = np.eye(mo)
            got[:m, :m] = Kz - Vd @ Vd.T + 0.5 * np.eye(m)
            judge(got, out, e_out, "pcov out")
            assert np.array_equal(got, got.T)


@pytest.mark.parametrize("n1,mw,mc,cb0,single", R.REMOVE_CASES)
def test_remove_reference(n1, mw, mc, cb0, single):
    """The float64 run of the recurrence keeps the orthogonal invariant within the bound the kernel is held to, the bound
    is under the cap of judge(), and its elements are within the cap of the long-double run."""
    Lt, Wp, Lw, Ww, beta = R.remove_problem(n1, mc, mw, cb0, single)
    kb1 = cb0 if single else (n1 - 1) // R.RB * R.RB
    Lf, Wf, _ = R.remove_blocks_ref(Lt, Wp, cb0, kb1, n1, mode="f64")
    Rs, B, gmax = R.remove_residual(Lt, Wp, Lf, Wf, cb0, kb1, n1, beta)
    assert B.max() <= 1e-10 * gmax
    assert (np.abs(Rs).astype(np.float64) <= B).all()
    Rl, _, _ = R.remove_residual(Lt, Wp, Lw, Ww, cb0, kb1, n1, beta)
    assert float(np.abs(Rl).max()) <= 2.0 ** -55 * gmax  # the long-double run keeps it to its own precision
    assert float(np.abs(Lf - Lw).max()) <= 1e-10 * float(np.abs(Lw).max())
    assert float(np.abs(Wf - Ww).max()) <= 1e-10 * float(np.abs(Ww).max())


def test_remove_reference_matches_remove_update():
    """remove_blocks_ref over all blocks is the recurrence of remove_ref.remove_update on the same removal."""
    import remove_ref
    n1, m = 200, 7
    Lt, W, L, rem = R.remove_operands(n1, m, full=True)
    L1, _, _ = R.remove_blocks_ref(Lt, W, 0, 128, n1, mode="f64")
    want = remove_ref.remove_update(L, rem, width=m)
    assert want.shape == (n1, n1) and np.abs(L1[:n1, :n1] - want).max() <= 1e-13 * np.abs(want).max()
