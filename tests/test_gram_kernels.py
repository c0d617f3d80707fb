"""The kernels that evaluate the similarity and the forecast-derivative kernels, in isolation (run with -m gpu on the MI355X
box): gram_kernel<CROSS, T>, gram_local_kernel<T>, kmatvec_kernel<RADIAL1>, each also as *_ev, kmatvec_finish_kernel and
prior_kernel of gram.hip; pgrad_kernel<4 | 8 | 16>, pgrad_kernel_ev and pgrad_final_kernel of pgrad.hip.

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h (gogp_test_gram_split, _gram_local,
_cross, _prior, _kmatvec, _pgrad).  tests/gram_ref.py holds the references, the model of the bounds and the cases:
- exact mode: inv_len = 0, c a power of two, dyadic discounts, an integer noise -- every live element is c d_ij (+ noise)
  BIT FOR BIT, the padding is the identity, and everything a launch must not write keeps its sentinel.  This pins which
  elements are written, from which pair, with which candidate's parameters;
- long-double mode: |got - ref| <= bound element by element, the bound from the model and the inputs alone;
- the one-radial-term fast paths against the generic path, bit for bit;
- sentinels (NaNs with a payload): every output before the launch, the rows n .. npad - 1 of X and of v, the rows
  m .. mpad - 1 of Z, alpha[n:], the columns n .. of Wt.  The guards keep them out of every result.
Every launch runs twice and must return the same bits.  The largest |got - ref| / bound per kernel is printed by the last
test (-s shows it)."""
import numpy as np
import pytest

import gram_ref as R
from cases import NAN32, NAN64

pytestmark = pytest.mark.gpu

F64, F32, LD = np.float64, np.float32, np.longdouble
RATIOS = {}


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def nan_of(dt):
    return NAN64 if np.dtype(dt) == F64 else NAN32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == F64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def sentinels(size, dt=F64):
    return np.full(size, nan_of(dt), dt)


def untouched(a):
    return bool((bits(a) == bits(np.array([nan_of(a.dtype)], a.dtype))[0]).all())


def twice(run):
    """The launch, run twice from the same inputs: the same bits."""
    a, b = run(), run()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert same_bits(x, y), "two launches differ"
    return a


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))


def judge(got, want, bound, what, family):
    """|got - want| <= bound element by element (equality where the bound is 0); records the worst ratio."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), "%s: %d non-finite values" % (what, int((~np.isfinite(got)).sum()))
    assert bound.max() <= 1e-10 * float(np.abs(want).max()) or got.dtype == F32 or np.abs(want).max() == 0, \
        "%s: the bound is too loose to judge by" % what
    err = np.abs(got.astype(LD) - want).astype(F64)
    bad = err > bound
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert not bad.any(), "%s: %d of %d outside the bound, worst |err| / bound = %g, first at %s" % (
        what, int(bad.sum()), got.size, ratio, tuple(np.argwhere(bad)[0]))
    note(family, ratio)
    return ratio


def matrix_of(flat, rows, ld, cols):
    """(the rows x cols window, everything else) of a flat array holding `rows` rows of ld."""
    body = flat[:rows * ld].reshape(rows, ld)
    return body[:, :cols], (body[:, cols:], flat[rows * ld:])


def rest_untouched(rest):
    return all(untouched(r) for r in rest if r.size)


def check_written(got, want, written, what, zeroed=None):
    """Exact mode: `want` bit for bit where written, +0 where zeroed, the sentinel everywhere else."""
    w = want.astype(got.dtype)
    assert np.array_equal(w.astype(F64), want), what + ": the exact reference does not fit the output type"
    bad = np.argwhere(written & (bits(got) != bits(w)))
    assert bad.size == 0, "%s: %d written elements differ, first at %s: %r vs %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], w[tuple(bad[0])])
    keep = ~written
    if zeroed is not None:
        assert (bits(got)[zeroed] == 0).all(), what + ": a block above the diagonal is not zero"
        keep = keep & ~zeroed
    assert untouched(got[keep]), "%s: %d elements outside the launch's tiles were written" % (
        what, int((bits(got[keep]) != bits(np.array([nan_of(got.dtype)], got.dtype))[0]).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact mode
# ---------------------------------------------------------------------------------------------------------------------
EXACT_VARIANTS = [("radial1", False), ("radial1", True), ("generic", False), ("generic", True)]
D_EXACT, AXIS_EXACT = 3, 1


def run_split_exact(gpm, npad, n, wcols, dt, which, ev, D=D_EXACT):
    axis = min(AXIS_EXACT, D - 1)
    kp, p = R.exact_kp(which, D, ev, axis), R.problem(D, npad, n, ev_axis=axis)
    ld = npad + 8
    K0 = sentinels(npad * ld + 5, dt)
    K = twice(lambda: gpm.gram_split_check(kp.hook(gpm), p["X"], n, npad, wcols, K0, ld, ev=ev))
    got, rest = matrix_of(K, npad, ld, npad)
    check_written(got, R.exact_gram(kp, p["x"], n, npad), R.split_written(npad), "split %s" % ((npad, n, wcols),))
    assert rest_untouched(rest), "the columns beyond npad or the tail were written"


@pytest.mark.parametrize("which,ev", EXACT_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("npad,n,wcols", R.SPLIT_SHAPES, ids=lambda v: str(v))
def test_split_gram_exact(gpm, npad, n, wcols, prec, which, ev):
    run_split_exact(gpm, npad, n, wcols, F64 if prec == 64 else F32, which, ev)


@pytest.mark.parametrize("prec", [64, 32])
def test_split_gram_exact_triangular_decode(gpm, prec):
    # 28 x 29 / 2 = 406 tiles in the second launch: the square-root decode of the tile index, and its correction loops
    npad, n, wcols = R.SPLIT_BIG
    run_split_exact(gpm, npad, n, wcols, F64 if prec == 64 else F32, "radial1", False, D=1)


@pytest.mark.parametrize("which", ["radial1", "generic"])
def test_split_gram_exact_candidates(gpm, which):
    npad, n, wcols, k, D = 320, 257, 128, 3, D_EXACT
    p = R.problem(D, npad, n, ev_axis=AXIS_EXACT)
    evs = [R.EXACT_EVENTS, R.EXACT_EVENTS[:1], R.EXACT_EVENTS[::-1]]
    kps = [R.KP(D, [dict(T, c=T["c"] * s) for T in R.EXACT_KERNELS[which]], evs[c], AXIS_EXACT, nv)
           for c, (s, nv) in enumerate([(1.0, 3.0), (2.0, 5.0), (0.5, 7.0)])]
    ld = npad + 8
    bstride = npad * ld + 6
    K0 = sentinels((k - 1) * bstride + npad * ld + 5)
    K = twice(lambda: gpm.gram_split_check([q.hook(gpm) for q in kps], p["X"], n, npad, wcols, K0, ld, ev=True,
                                           bstride=bstride))
    wants = [R.exact_gram(q, p["x"], n, npad) for q in kps]
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[0], wants[2] * 2)
    for c in range(k):
        got, rest = matrix_of(K[c * bstride:(c + 1) * bstride] if c < k - 1 else K[c * bstride:], npad, ld, npad)
        check_written(got, wants[c], R.split_written(npad), "candidate %d" % c)
        assert rest_untouched(rest), "candidate %d: written outside its matrix" % c


LOCAL_CASES = [(sh, Pr, Pc) for sh in (6, 7) for (Pr, Pc) in R.LOCAL_GRIDS] + [(9, 2, 1)]


@pytest.mark.parametrize("which,ev", [("radial1", True), ("generic", False)], ids=lambda v: str(v))
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("nb_shift,Pr,Pc", LOCAL_CASES, ids=lambda v: str(v))
def test_local_gram_exact(gpm, nb_shift, Pr, Pc, prec, which, ev):
    dt = F64 if prec == 64 else F32
    nb, NB = 1 << nb_shift, R.S.num_tiles(Pr, Pc, 2 if nb_shift < 9 else 1)
    npad = NB * nb
    n = npad - nb // 2 - 17 if nb_shift > 6 else npad - 64 - 17  # ragged inside a tile; at nb = 64 a whole tile of padding
    D = 2
    kp, p = R.exact_kp(which, D, ev, 1), R.problem(D, npad, n, ev_axis=1)
    G = R.exact_gram(kp, p["x"], n, npad)
    back = np.full((npad, npad), np.nan)
    seen_upper_tile = False
    for pr in range(Pr):
        for pc in range(Pc):
            want, written, zeroed = R.local_cut(G, nb, Pr, Pc, pr, pc)
            mrows, ncols = want.shape
            ld = ncols + 8
            K0 = sentinels(mrows * ld + 5, dt)
            K = twice(lambda: gpm.gram_local_check(kp.hook(gpm), p["X"], n, npad, mrows, ncols, (pr, Pr, pc, Pc), K0, ld,
                                                   nb_shift=nb_shift, ev=ev))
            got, rest = matrix_of(K, mrows, ld, ncols)
            check_written(got, want, written, "rank (%d, %d)" % (pr, pc), zeroed)
            assert rest_untouched(rest)
            seen_upper_tile |= bool((~written & ~zeroed).any())
            gr, gc = R.S.global_rows(NB, nb, Pr, pr), R.S.global_rows(NB, nb, Pc, pc)
            blk = back[np.ix_(gr, gc)]
            assert np.isnan(blk).all(), "two ranks hold the same element"
            back[np.ix_(gr, gc)] = np.where(written, got.astype(F64), np.nan)
    assert seen_upper_tile == (nb >= 128), "the untouched upper tile inside a diagonal block exists from nb = 128 on"
    low = R.split_written(npad)
    assert np.array_equal(back[low], G[low]) and np.isnan(back[~low]).all(), "the ranks' tiles do not reassemble the matrix"


@pytest.mark.parametrize("which,ev", [("generic", True), ("radial1", False)], ids=lambda v: str(v))
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("m", R.CROSS_M)
@pytest.mark.parametrize("n", R.CROSS_N)
def test_cross_exact(gpm, n, m, prec, which, ev):
    dt = F64 if prec == 64 else F32
    npad, mpad, D = -(-n // 64) * 64, -(-m // 64) * 64, D_EXACT
    kp, p = R.exact_kp(which, D, ev, AXIS_EXACT), R.problem(D, npad, n, m, mpad, AXIS_EXACT)
    ld = npad + 8
    K0 = sentinels(mpad * ld + 5, dt)
    K = twice(lambda: gpm.cross_check(kp.hook(gpm), p["X"], n, npad, p["Z"], m, mpad, K0, ld, ev=ev))
    got, rest = matrix_of(K, mpad, ld, npad)
    want = np.zeros((mpad, npad))
    want[:m, :n] = sum(T["c"] for T in kp.terms) * R.discount(kp.events, p["z"][:, kp.ev_axis], p["x"][:, kp.ev_axis])
    check_written(got, want, np.ones((mpad, npad), bool), "cross n=%d m=%d" % (n, m))
    assert rest_untouched(rest), "the columns beyond npad or the tail were written"


KMATVEC_VARIANTS = [("radial1", 1), ("radial1", 0), ("generic", 0)]


@pytest.mark.parametrize("ev", [False, True])
@pytest.mark.parametrize("which,radial1", KMATVEC_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("npad,n", [(64, 1), (128, 100), (320, 257)], ids=lambda v: str(v))
def test_kmatvec_exact(gpm, npad, n, which, radial1, ev):
    D, ntile = D_EXACT, npad // 64
    kp, p = R.exact_kp(which, D, ev, AXIS_EXACT), R.problem(D, npad, n, ev_axis=AXIS_EXACT, integer=True)
    G = R.exact_gram(kp, p["x"], n, npad)[:n, :n]
    v, y = p["v"][:n], p["y"][:n]
    assert np.abs(G).sum(1).max() * 8 < 2.0 ** 40  # every partial sum is a dyadic number far below 2^53: exact in any order
    col_tile = np.arange(n) // 64

    def expect(nslab, t0, t1, share):
        part = np.zeros((nslab, npad))
        for s, (a, b) in enumerate(R.slab_columns(npad, nslab, t0, t1, share)):
            sel = (col_tile >= a) & (col_tile < b)
            part[s, :n] = G[:, sel] @ v[sel]
        return part

    def run(nslab, yy, part_idx=0, nparts=1):
        part0, out0 = sentinels(nslab * npad + 3), sentinels(npad + 3)
        part, out = twice(lambda: gpm.kmatvec_check(kp.hook(gpm), p["X"], n, npad, p["v"], yy, part0, nslab, out0, part_idx,
                                                    nparts, radial1=bool(radial1), ev=ev))
        assert untouched(part[nslab * npad:]) and untouched(out[npad:])
        return part[:nslab * npad].reshape(nslab, npad), out[:npad]

    for nslab in (1, 3, 8):
        part, r = run(nslab, p["y"])
        want = expect(nslab, 0, ntile, False)
        assert same_bits(part, want), "residual: the slabs' sums (nslab %d)" % nslab
        wr = np.zeros(npad)
        wr[:n] = y - G @ v
        assert same_bits(r, wr), "residual: r = y - K v, zero from row n on (nslab %d)" % nslab
        for nparts in (1, 2, 3):
            total = np.zeros(npad)
            for part_idx in range(nparts):
                t0, t1 = R.share_tiles(npad, part_idx, nparts)
                part, out = run(nslab, None, part_idx, nparts)
                want = expect(nslab, t0, t1, True)
                assert same_bits(part, want), "share %d of %d: the slabs' sums (nslab %d)" % (part_idx, nparts, nslab)
                assert same_bits(out, want.sum(0)), "share %d of %d (nslab %d)" % (part_idx, nparts, nslab)
                total += out
            whole = np.zeros(npad)
            whole[:n] = G @ v
            assert same_bits(total, whole), "the shares do not add up to the whole"
    if ntile <= 2:
        assert R.share_tiles(npad, 2, 3) == (ntile, ntile)  # a share with no tiles was among them


# ---------------------------------------------------------------------------------------------------------------------
# 2. long-double mode, 3. the fast path is the generic path
# ---------------------------------------------------------------------------------------------------------------------
def ld_setup(case):
    sh = R.LD_SHAPE
    kp = R.kp_of(case)
    p = R.problem(case[1], sh["npad"], sh["n"], sh["m"], sh["mpad"], case[3] if case[2] else -1)
    return kp, p, sh["npad"], sh["n"], sh["m"], sh["mpad"], bool(case[2])


def launch_split(gpm, kp, p, n, npad, dt, ev, wcols=128):
    K0 = sentinels(npad * npad, dt)
    return twice(lambda: gpm.gram_split_check(kp.hook(gpm), p["X"], n, npad, wcols, K0, npad, ev=ev)).reshape(npad, npad)


def launch_cross(gpm, kp, p, n, npad, Z, m, mpad, dt, ev):
    K0 = sentinels(mpad * npad, dt)
    return twice(lambda: gpm.cross_check(kp.hook(gpm), p["X"], n, npad, Z, m, mpad, K0, npad, ev=ev)).reshape(mpad, npad)


def launch_kmatvec(gpm, kp, p, n, npad, y, radial1, ev, nslab=3, part_idx=0, nparts=1):
    part0, out0 = sentinels(nslab * npad), sentinels(npad)
    return twice(lambda: gpm.kmatvec_check(kp.hook(gpm), p["X"], n, npad, p["v"], y, part0, nslab, out0, part_idx, nparts,
                                           radial1=radial1, ev=ev))[1]


@pytest.mark.parametrize("case", R.LD_CASES, ids=R.case_id)
def test_gram_long_double(gpm, case):
    kp, p, npad, n, m, mpad, ev = ld_setup(case)
    fam = "ev" if ev else "plain"
    low = R.split_written(npad)
    for dt in (F64, F32):
        G, E = R.padded_gram(kp, p["x"], n, npad, out32=dt == F32)
        K = launch_split(gpm, kp, p, n, npad, dt, ev)
        assert untouched(K[~low]), "split: an upper tile was written"
        judge(np.where(low, K, 0), np.where(low, G, 0), np.where(low, E, 0), "split %s" % dt.__name__,
              "gram_kernel<false,%s> %s" % (dt.__name__, fam))
        # rank (1, 0) of a 2 x 1 grid with blocks of 128: a full block and a diagonal one with its untouched upper tile
        want, written, zeroed = R.local_cut(G, 128, 2, 1, 1, 0)
        bound = R.local_cut(E, 128, 2, 1, 1, 0)[0]
        K0 = sentinels(want.size, dt)
        Kl = twice(lambda: gpm.gram_local_check(kp.hook(gpm), p["X"], n, npad, want.shape[0], want.shape[1], (1, 2, 0, 1), K0,
                                                want.shape[1], nb_shift=7, ev=ev)).reshape(want.shape)
        assert untouched(Kl[~written & ~zeroed]) and (bits(Kl)[zeroed] == 0).all()
        judge(np.where(written, Kl, 0), np.where(written, want, 0), np.where(written, bound, 0), "local %s" % dt.__name__,
              "gram_local_kernel<%s> %s" % (dt.__name__, fam))
        C, EC = R.padded_cross(kp, p["x"], n, npad, p["z"], m, mpad, out32=dt == F32)
        Ks = launch_cross(gpm, kp, p, n, npad, p["Z"], m, mpad, dt, ev)
        assert (bits(Ks[m:]) == 0).all() and (bits(Ks[:, n:]) == 0).all(), "cross: the padding is not zero"
        judge(Ks, C, EC, "cross %s" % dt.__name__, "gram_kernel<true,%s> %s" % (dt.__name__, fam))


@pytest.mark.parametrize("case", R.LD_CASES, ids=R.case_id)
def test_kmatvec_long_double(gpm, case):
    kp, p, npad, n, _, _, ev = ld_setup(case)
    fam = "ev" if ev else "plain"
    want_r, e_r = R.matvec(kp, p["x"], n, p["v"], p["y"])
    t0, t1 = R.share_tiles(npad, 1, 2)
    cols = np.arange(t0 * 64, min(t1 * 64, n))
    want_s, e_s = R.matvec(kp, p["x"], n, p["v"], None, cols)
    for radial1 in ([False, True] if kp.radial1 else [False]):
        name = "kmatvec_kernel<%s> %s" % (str(radial1).lower(), fam)
        r = launch_kmatvec(gpm, kp, p, n, npad, p["y"], radial1, ev)  # D = 62 .. 64: more than 64 KB of dynamic LDS
        assert (bits(r[n:]) == 0).all(), "residual: rows >= n are not zero"
        judge(r[:n], want_r, e_r, "residual radial1=%d" % radial1, name)
        s = launch_kmatvec(gpm, kp, p, n, npad, None, radial1, ev, 3, 1, 2)
        assert (bits(s[n:]) == 0).all()
        judge(s[:n], want_s, e_s, "share 1 of 2 radial1=%d" % radial1, name)


RADIAL1_CASES = [c for c in R.LD_CASES if R.kp_of(c).radial1]


@pytest.mark.parametrize("case", RADIAL1_CASES, ids=R.case_id)
def test_fast_path_is_the_generic_path(gpm, case):
    """The one-radial-term paths of gram_kernel<false> and kmatvec_kernel<true> claim the same operations in the same order
    per pair as simil_value(): the split Gram matrix equals the cross kernel with Z = X (always the generic path) bit for
    bit below the diagonal, and kmatvec with radial1 = 1 equals radial1 = 0."""
    kp, p, npad, n, _, _, ev = ld_setup(case)
    Zx = p["X"][:npad * kp.ndim].copy()
    strict = np.tril(np.ones((npad, npad), bool), -1)
    strict[n:] = False
    for dt in (F64, F32):
        K = launch_split(gpm, kp, p, n, npad, dt, ev)
        Ks = launch_cross(gpm, kp, p, n, npad, Zx, n, npad, dt, ev)
        diff = strict & (bits(K) != bits(Ks))
        assert not diff.any(), "%d pairs differ between the fast and the generic path, first at %s" % (
            int(diff.sum()), tuple(np.argwhere(diff)[0]))
        # gram_local_kernel's copy of the fast path: rank (1, 0) of a 2 x 1 grid holds the same bits as the split launch
        want, written, _ = R.local_cut(K, 128, 2, 1, 1, 0)
        K0 = sentinels(want.size, dt)
        Kl = gpm.gram_local_check(kp.hook(gpm), p["X"], n, npad, want.shape[0], want.shape[1], (1, 2, 0, 1), K0, want.shape[1],
                                  nb_shift=7, ev=ev).reshape(want.shape)
        assert written.any() and (bits(Kl)[written] == bits(want)[written]).all(), "the local and the split launch differ"
    for y in (p["y"], None):
        a = launch_kmatvec(gpm, kp, p, n, npad, y, True, ev)
        b = launch_kmatvec(gpm, kp, p, n, npad, y, False, ev)
        assert same_bits(a, b), "kmatvec: radial1 = 1 and radial1 = 0 differ"


# ---------------------------------------------------------------------------------------------------------------------
# 4. the prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(R.RADIAL) + ["periodic", "max_terms", "hyperpriors", "ard"])
@pytest.mark.parametrize("m", R.PRIOR_M)
def test_prior(gpm, m, kind):
    D = 5
    kp, p = R.KP(D, R.terms_of(kind, D)), R.problem(D, 64, 1, m, -(-m // 64) * 64)
    out = twice(lambda: gpm.prior_check(kp.hook(gpm), p["Z"], m, sentinels(m + 3)))
    want = F64(0.0)
    for T in kp.terms:  # s = 0, so f = 1 for every kind: the float64 sum of the output scales in term order, from 0
        want = want + F64(T["c"])
    assert want == F64(R.prior_values(kp))
    assert same_bits(out[:m], np.full(m, want)), "prior: not the sum of the output scales"
    assert untouched(out[m:])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the forecast derivatives
# ---------------------------------------------------------------------------------------------------------------------
def run_pgrad(gpm, kp, p, n, npad, m, ld, ev, alpha=None, Wt=None, sigma=None):
    D = kp.ndim
    alpha = p["alpha"] if alpha is None else alpha
    Wt = p["Wt"] if Wt is None else Wt
    sigma = p["sigma"] if sigma is None else sigma
    nslab, _ = gpm.pgrad_slabs(npad, m)
    assert (nslab, _) == R.pgrad_slabs(npad, m)
    md = m * D
    part0, dmu0, dsig0 = sentinels(2 * nslab * md + 3), sentinels(md + 3), sentinels(md + 3)
    part, dmu, dsig = twice(lambda: gpm.pgrad_check(kp.hook(gpm), p["X"], n, npad, p["Z"], m, alpha, Wt, ld, sigma, part0,
                                                    dmu0, dsig0, ev=ev))
    assert untouched(part[2 * nslab * md:]) and untouched(dmu[md:]) and untouched(dsig[md:])
    part = part[:2 * nslab * md].reshape(2, nslab, m, D)
    assert np.isfinite(part).all(), "a slab's partial sums were not written"
    # pgrad_final_kernel: the slabs in order from 0, then (-2 b) / (2 sigma) -- the same IEEE operations here
    a, b = np.zeros((m, D)), np.zeros((m, D))
    for sl in range(nslab):
        a, b = a + part[0, sl], b + part[1, sl]
    dmu, dsig = dmu[:md].reshape(m, D), dsig[:md].reshape(m, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert same_bits(dmu, a) and same_bits(dsig, (-2.0 * b) / (2.0 * sigma[:m, None])), "pgrad_final_kernel"
    return dmu, dsig


@pytest.mark.parametrize("case", R.PGRAD_CASES, ids=lambda c: R.case_id(c[:4]) + "-m%d-%d/%d" % (c[4], c[6], c[5]))
def test_pgrad_long_double(gpm, case):
    kind, D, nev, axis, m, npad, n = case
    kp = R.kp_of(case[:4])
    ld = npad + 8
    p = R.pgrad_problem(D, npad, n, m, ld, axis if nev else -1)
    dmu, dsig = run_pgrad(gpm, kp, p, n, npad, m, ld, bool(nev))
    w_dmu, e_dmu, w_dsig, e_dsig = R.pgrad_sums(kp, p["x"], n, p["z"], m, p["alpha"], p["Wt"].reshape(m, ld), p["sigma"])
    fam = "pgrad_kernel%s<%d>" % ("_ev" if nev else "", 4 if D <= 4 else 8 if D <= 8 else 16)
    judge(dmu, w_dmu, e_dmu, "dmu", fam)
    judge(dsig, w_dsig, e_dsig, "dsigma", fam)


@pytest.mark.parametrize("D,ev", [(3, False), (8, True), (17, False)])
def test_pgrad_single_pairs(gpm, D, ev):
    """alpha = e_i and Wt[j] = e_i: every sum is one pair, which pins which row meets which test point."""
    npad, n, m = 256, 193, 5
    ld = npad + 8
    kp = R.kp_of(("matern52", D, 3 if ev else 0, D - 1))
    p = R.pgrad_problem(D, npad, n, m, ld, D - 1 if ev else -1)
    for i in (0, 63, 64, n - 1):
        alpha, Wt = np.full(npad, NAN64), np.full((m, ld), NAN64)
        alpha[:n], Wt[:, :n] = 0.0, 0.0
        alpha[i], Wt[:, i] = 1.0, 1.0
        dmu, dsig = run_pgrad(gpm, kp, p, n, npad, m, ld, ev, alpha, Wt.reshape(-1))
        w_dmu, e_dmu, w_dsig, e_dsig = R.pgrad_sums(kp, p["x"], n, p["z"], m, alpha, Wt, p["sigma"])
        assert np.abs(w_dmu).max(1).min() > 0, "a pair without a derivative pins nothing"
        judge(dmu, w_dmu, e_dmu, "dmu, the pair with row %d" % i, "pgrad single pairs")
        judge(dsig, w_dsig, e_dsig, "dsigma, the pair with row %d" % i, "pgrad single pairs")


def test_pgrad_nonpositive_sigma(gpm):
    """sigma is not clamped: a row with sigma_j < 0 flips the sign, sigma_j = 0 is what the division yields."""
    D, npad, n, m = 4, 64, 40, 5
    kp = R.kp_of(("normal", D, 0, 0))
    p = R.pgrad_problem(D, npad, n, m, npad)
    sigma = p["sigma"].copy()
    sigma[1], sigma[3] = -0.75, 0.0
    _, dsig = run_pgrad(gpm, kp, p, n, npad, m, npad, False, sigma=sigma)  # (which holds dsigma to the division's bits)
    _, _, want, e = R.pgrad_sums(kp, p["x"], n, p["z"], m, p["alpha"], p["Wt"].reshape(m, npad), sigma)
    live = np.array([0, 1, 2, 4])
    judge(dsig[live], want[live], e[live], "dsigma with a negative sigma", "pgrad_final_kernel")
    _, _, wb, eb = R.pgrad_sums(kp, p["x"], n, p["z"], m, p["alpha"], p["Wt"].reshape(m, npad), np.ones(m))  # -b
    assert (np.abs(wb[3]).astype(F64) > eb[3]).all(), "a sum too close to zero to know its sign"
    assert np.isinf(dsig[3]).all() and np.array_equal(np.sign(dsig[3]), np.sign(wb[3]).astype(F64))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the report
# ---------------------------------------------------------------------------------------------------------------------
def test_zz_report_ratios():
    """The largest |got - ref| / bound per kernel seen in this run (always passes; -s shows it)."""
    for f in sorted(RATIOS):
        print("KERNEL %-36s max |got - ref| / bound = %.3f" % (f, RATIOS[f]))
