"""The kernels behind Append, Remove, ProduceGradient's skinny product and ProduceCovariance, in isolation (run with -m gpu
on the MI355X box): append_gram_kernel and append_commit_kernel (append.hip), the gather, W, snapshot and block kernels
of remove.hip, bwd_panel_kernel (pgrad.hip) and pcov_syrk_kernel / pcov_final_kernel(_ev) (pcov.hip).

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h, which copy whole host arrays to
the device and back.  Three kinds of check, as in tests/test_substitution_kernels.py (tests/update_kernels_ref.py holds
the references):
- exact: integer / dyadic operands whose partial sums stay far below 2^53 in any order -- BIT FOR BIT.  The similarity is
  kept exact by inv_len = 0 (simil_value returns c whatever the points), so the kernels that evaluate it are exact too;
  append_commit gets S = L0 L0^T with an integer L0, whose every square root, quotient and fma is exact;
- full mantissa: random operands against a long-double run, |got - want| <= e with e = gamma_K |A| |B| for the products
  (judge() asserts max(e) <= 1e-10 max |want|, so the bound cannot hide a failure).  remove_block is held to the
  orthogonal invariant Z' Z'^T = Z Z^T of its reflectors, evaluated in long double, within the row-wise bound of an fp64
  evaluation in any order (update_kernels_ref.remove_residual, which says why a running bound on the ELEMENTS cannot stay
  below that cap: it grows 3^k where the error does not grow), and its elements to the long-double run of the recurrence
  of remove_ref.remove_update within that cap itself, 1e-10 max |want|;
- sentinels: NaNs with a payload in everything a launch must not read or write; they come back bit for bit, and a single
  check fails on any non-finite result.

Every test prints its worst |err| / e.
"""
import numpy as np
import pytest

import update_kernels_ref as R
from cases import NAN64
from test_substitution_kernels import judge, same_bits

pytestmark = pytest.mark.gpu

P, RB, AP = R.P, R.RB, R.APPEND_PART
NAN_BITS = np.array([NAN64]).view(np.uint64)[0]


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def sentinels(n):
    return np.full(n, NAN64)


def untouched(a, what):
    """Every element still holds the sentinel, bit for bit."""
    bad = np.flatnonzero(np.ascontiguousarray(a).reshape(-1).view(np.uint64) != NAN_BITS)
    assert bad.size == 0, "%s: %d of %d sentinels overwritten, first at %d" % (what, bad.size, a.size, bad[0])


def kparams(gpm, ev_given=True):
    """One NORMAL term with inv_len = 0: k = c exactly (times the pair's dyadic event discount in the ev instances)."""
    return gpm.kparams(2, [dict(kind=0, c=R.C_EXACT, inv_len=0.0)], noise_var=R.NOISE_EXACT,
                       events=R.EVENTS if ev_given else (), ev_axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# append_gram_kernel
# ---------------------------------------------------------------------------------------------------------------------
def gram_id(c):
    npc, dn, m, rows = c
    return "npc%d-n%d-m%d%s" % (npc, npc - dn, m, "-rows" if rows else "")


def test_every_layout_is_named():
    first, second = set(), set()
    for _, _, m, rows in R.GRAM_CASES:
        if rows:
            first.add(("rows", 0))
            continue
        first.add(R.solution_layout(0, min(m, 32)))
        if m > 32:
            second.add(R.solution_layout(32, m - 32))
    C, Pd, G = R.TS_SOL_COMPACT, R.TS_SOL_PAIRED, R.TS_SOL_GRANULE
    assert first == {("rows", 0), (G, 1), (C, 2), (C, 4), (C, 8), (Pd, 16), (Pd, 32)}, sorted(first, key=str)
    assert second == {(C, 1), (C, 2), (C, 4), (C, 8), (Pd, 16), (Pd, 32)}, sorted(second)


@pytest.mark.parametrize("npc,dn,m,rows", R.GRAM_CASES, ids=[gram_id(c) for c in R.GRAM_CASES])
def test_append_gram(gpm, npc, dn, m, rows):
    n, ns, ld = npc - dn, npc // P, npc + 8
    written = R.gram_written(m)
    worst = 0.0
    for exact in (True, False):
        V, z = R.gram_problem(npc, exact)
        V = V[:, :m]
        s0, s1, m0 = R.gram_sources(V, rows)
        part, Lnew = gpm.append_gram_check(s0, s1, m0, m, npc, n, z, sentinels((ns + 1) * AP + 3), sentinels((m + 2) * ld), ld)
        G, dots, LT, eG, ed = R.gram_ref(V, z, n, exact)
        for s in range(ns):
            slot = part[s * AP:(s + 1) * AP]
            Gs = slot[:4096].reshape(64, 64)
            worst = max(worst, judge(Gs[written], G[s][written], None if exact else eG[s][written], "V^T V, slab %d" % s))
            worst = max(worst, judge(slot[4096:], dots[s], None if exact else ed[s], "V^T z, slab %d" % s))
            untouched(Gs[~written], "the tiles of part above the diagonal tile row and below tile row ceil(m / 16)")
        untouched(part[ns * AP:], "part behind the last slab")
        Lv = Lnew.reshape(m + 2, ld)
        assert np.isfinite(Lv[:m, :n]).all() and same_bits(Lv[:m, :n], LT), "the transposed rows are a copy, bit for bit"
        untouched(Lv[:m, n:], "Lnew columns k >= n")
        untouched(Lv[m:], "Lnew rows >= m")
    print("RATIO append_gram %s %.4f" % (gram_id((npc, dn, m, rows)), worst))


# ---------------------------------------------------------------------------------------------------------------------
# append_commit_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,nslab,n,ev", R.COMMIT_CASES,
                         ids=["m%d-s%d-n%d-%s" % (m, s, n, "ev" if e else "plain") for m, s, n, e in R.COMMIT_CASES])
def test_append_commit_exact(gpm, m, nslab, n, ev):
    pr = R.commit_problem(m, nslab, ev, 100 * m + nslab)
    ld = n + m + 5
    Lnew, z2, info = gpm.append_commit_check(kparams(gpm), pr["X2"].reshape(-1), pr["y2"], m, n, pr["part"], nslab,
                                             sentinels((m + 1) * ld), ld, sentinels(m + 3), 0, ev)
    assert info == 0
    Lv = Lnew.reshape(m + 1, ld)
    judge(Lv[:m, n:n + m], pr["L0"], None, "L22")
    judge(z2[:m], pr["z0"], None, "z2")
    untouched(Lv[:m, :n], "Lnew left of column n")
    untouched(Lv[:m, n + m:], "Lnew right of column n + m - 1")
    untouched(Lv[m:], "Lnew rows >= m")
    untouched(z2[m:], "z2 behind m")
    print("RATIO append_commit m%d s%d n%d ev%d 0.0000 (bit for bit)" % (m, nslab, n, ev))


@pytest.mark.parametrize("m,pivot,how", R.NOTPD_CASES, ids=["m%d-p%d-%s" % c for c in R.NOTPD_CASES])
def test_append_commit_not_positive_definite(gpm, m, pivot, how):
    """A numerical status, not a fault: info = n + pivot + 1 (an info already set is kept), nothing else is written."""
    n, nslab = 300, 3
    pr = R.commit_problem(m, nslab, True, 7 * m + pivot, bad=(pivot, how))
    ld = n + m + 5
    for info_in in (0, 7):
        Lnew, z2, info = gpm.append_commit_check(kparams(gpm), pr["X2"].reshape(-1), pr["y2"], m, n, pr["part"], nslab,
                                                 sentinels((m + 1) * ld), ld, sentinels(m + 3), info_in, True)
        assert info == (info_in or n + pivot + 1), (info, info_in, n + pivot + 1)
        untouched(Lnew, "Lnew after a failed block")
        untouched(z2, "z2 after a failed block")
    print("RATIO append_commit notpd m%d p%d %s 0.0000 (bit for bit)" % (m, pivot, how))


# ---------------------------------------------------------------------------------------------------------------------
# bwd_panel_kernel
# ---------------------------------------------------------------------------------------------------------------------
PANEL_CASES = [(r,) + s for s in R.PANEL_SHAPES for r in R.PANEL_ROWS16]


@pytest.mark.parametrize("rows16,K,ncols,ldb,tri,sub", PANEL_CASES,
                         ids=["r%d-K%d-c%d-ldb%d-%s" % (c[0], c[1], c[2], c[3], "tri" if c[4] else "sub") for c in PANEL_CASES])
def test_bwd_panel(gpm, rows16, K, ncols, ldb, tri, sub):
    rows = R.panel_rows(rows16)
    lda, ldc, a_off, b_off, c_off = K + 4, ncols + 4, 8, 16, 4
    worst = 0.0
    for exact in (True, False):
        rng = np.random.default_rng(4000 + rows16 + K + ncols + exact)
        draw = (lambda s: rng.integers(-1, 2, s).astype(np.float64)) if exact else rng.standard_normal
        A, B, C = sentinels(a_off + rows * lda + 3), sentinels(b_off + K * ldb + 3), sentinels(c_off + (rows + 1) * ldc)
        Av = A[a_off:a_off + rows * lda].reshape(rows, lda)
        Bv = B[b_off:b_off + K * ldb].reshape(K, ldb)
        Cv = C[c_off:c_off + rows * ldc].reshape(rows, ldc)
        Av[:, :K] = draw((rows, K))
        Bd = draw((K, ncols))
        if tri:  # zero above the diagonal, element by element; the rows k < j0 of every 64-column block are never read
            Bd = np.tril(Bd)
            Bv[:, :ncols] = Bd
            for j0 in range(64, ncols, 64):
                Bv[:j0, j0:j0 + 64] = NAN64
        else:
            Bv[:, :ncols] = Bd
        C0 = (rng.integers(-8, 9, (rows, ncols)).astype(np.float64) if exact else rng.standard_normal((rows, ncols)))
        if sub:
            Cv[:, :ncols] = C0
        got = gpm.bwd_panel_check(rows16, A, a_off, lda, B, b_off, ldb, C, c_off, ldc, ncols, K, tri, sub)
        want, e = R.panel_ref(Av[:, :K].copy(), Bd, C0, sub, exact)
        gv = got[c_off:c_off + rows * ldc].reshape(rows, ldc)
        worst = max(worst, judge(gv[:, :ncols], want, e, "C"))
        untouched(gv[:, ncols:], "C right of ncols")
        untouched(got[:c_off], "C before the offset")
        untouched(got[c_off + rows * ldc:], "C behind the last row")
    print("RATIO bwd_panel r%d K%d c%d %s %.4f" % (rows16, K, ncols, "tri" if tri else "sub", worst))


# ---------------------------------------------------------------------------------------------------------------------
# launch_pcov: pcov_syrk_kernel and pcov_final_kernel(_ev)
# ---------------------------------------------------------------------------------------------------------------------
def test_pcov_slab_counts(gpm):
    for (m, npad, ncu), want in R.PCOV_SLABS.items():
        assert gpm.pcov_slabs(npad, m, ncu) == want == R.slabs_ref(npad, m, ncu), (m, npad, ncu)


@pytest.mark.parametrize("m,npad,ncu,mo,ev", R.PCOV_CASES,
                         ids=["m%d-n%s-cu%d-mo%d-%s" % (c[0], c[1], c[2], c[3], "ev" if c[4] else "plain") for c in R.PCOV_CASES])
def test_pcov(gpm, m, npad, ncu, mo, ev):
    Z = R.points(m, 600 + m)
    Kz = R.simil_exact(Z[:, 1], ev)
    diag_add, ldo = 0.5, mo + 3
    kp = kparams(gpm)
    worst = 0.0
    for exact in ((True, False) if npad else (True,)):
        out0 = sentinels((mo + 1) * ldo)
        if npad is None:
            part, out = gpm.pcov_check(kp, Z.reshape(-1), m, None, 0, 0, ncu, None, out0, mo, ldo, diag_add, ev)
            _, want, _, e_out = R.pcov_ref(None, Kz, diag_add, 0, 0, mo, True)
        else:
            nslab, cps = gpm.pcov_slabs(npad, m, ncu)
            assert (nslab, cps) == R.slabs_ref(npad, m, ncu)
            rng = np.random.default_rng(5000 + m + npad + exact)
            Vd = rng.integers(-1, 2, (m, npad)).astype(np.float64) if exact else rng.standard_normal((m, npad))
            ld = npad + 2
            Vt = sentinels((m + 1) * ld)  # rows >= m and the columns from npad on are never read
            Vt.reshape(m + 1, ld)[:m, :npad] = Vd
            npairs = len(R.pair_list(m))
            part, out = gpm.pcov_check(kp, Z.reshape(-1), m, Vt, ld, npad, ncu, sentinels(nslab * npairs * 4096 + 7), out0,
                                       mo, ldo, diag_add, ev)
            pw, want, e_part, e_out = R.pcov_ref(Vd, Kz, diag_add, nslab, cps, mo, exact)
            worst = max(worst, judge(part[:pw.size].reshape(pw.shape), pw, e_part, "the slab parts"))
            untouched(part[pw.size:], "part behind the last slab")
        ov = out.reshape(mo + 1, ldo)
        worst = max(worst, judge(ov[:mo, :mo], want, None if exact else e_out, "out"))
        assert same_bits(ov[:mo, :mo], np.ascontiguousarray(ov[:mo, :mo].T)), "out and its transpose differ in bits"
        if mo > m:
            I = np.eye(mo)
            assert same_bits(ov[m:mo, :mo], I[m:]) and same_bits(np.ascontiguousarray(ov[:mo, m:mo]), I[:, m:])
        untouched(ov[:mo, mo:], "out right of mo")
        untouched(ov[mo:], "out below mo")
    print("RATIO pcov m%d n%s cu%d mo%d ev%d %.4f" % (m, npad, ncu, mo, ev, worst))


# ---------------------------------------------------------------------------------------------------------------------
# remove.hip
# ---------------------------------------------------------------------------------------------------------------------
def removal(n1, m, seed):
    """(src flat with a sentinel upper triangle, ld0, map, rem) of n1 rows kept out of n1 + m of a 768-row factor."""
    rng = np.random.default_rng(seed)
    n0, ld0 = n1 + m, 768
    src = rng.standard_normal((n0, ld0))
    src[np.triu_indices(n0, 1, ld0)] = NAN64  # neither kernel reads above the diagonal of the old factor
    rem = np.sort(rng.choice(n0, m, replace=False)).astype(np.int32)
    map_ = np.setdiff1d(np.arange(n0), rem).astype(np.int32)
    return src, ld0, map_, rem


@pytest.mark.parametrize("n1", R.REMOVE_N1)
def test_remove_gather(gpm, n1):
    src, ld0, map_, _ = removal(n1, 40, 70 + n1)
    dst0 = sentinels(512 * 512)
    got = gpm.remove_gather_check(src.reshape(-1), ld0, map_, n1, dst0, 512)
    want = R.gather_ref(src, map_, n1, 512, dst0.reshape(512, 512))
    assert same_bits(got.reshape(512, 512), want)
    print("RATIO remove_gather n%d 0.0000 (bit for bit)" % n1)


@pytest.mark.parametrize("r0", [0, 128])
@pytest.mark.parametrize("mw,mc", [(4, 1), (4, 4), (32, 5), (32, 32)])
@pytest.mark.parametrize("n1", R.REMOVE_N1)
def test_remove_w(gpm, n1, mw, mc, r0):
    src, ld0, map_, rem = removal(n1, mc, 90 + n1 + mc)
    W0 = sentinels(mw * 512 + 5)
    got = gpm.remove_w_check(src.reshape(-1), ld0, map_, rem, mc, mw, r0, n1, 512, W0)
    want = R.w_ref(src, map_, rem, mc, mw, r0, n1, 512, W0[:mw * 512].reshape(mw, 512))
    assert same_bits(got[:mw * 512].reshape(mw, 512), want)
    untouched(got[mw * 512:], "W behind the last column")
    print("RATIO remove_w n%d mw%d mc%d r%d 0.0000 (bit for bit)" % (n1, mw, mc, r0))


def device_operands(Lt, Wp, cb0, n1):
    """L, W and the snapshot as a launch from block cb0 may see them: sentinels in the columns left of cb0, above the
    diagonal, in the rows from n1 on of L, in the rows of W above cb0 and behind the last block; zeros in the rows of W
    between n1 and the end of its block (remove_w leaves them so, and the block's workgroups read them)."""
    npad = Lt.shape[0]
    mw = Wp.shape[0]
    L = sentinels(npad * npad).reshape(npad, npad)
    low = np.tril(np.ones((npad, npad), bool))
    low[:cb0] = low[n1:] = False
    low[:, :cb0] = False
    L[low] = Lt[low]
    W = sentinels(mw * npad + 5)
    Wv = W[:mw * npad].reshape(mw, npad)
    Wv[:, cb0:n1] = Wp[:, cb0:n1]
    Wv[:, n1:-(-n1 // RB) * RB] = 0.0
    return L, low, W, sentinels(npad * RB + 3)


def check_blocks(gpm, L0, low, W0, snap0, Lt, Wp, mw, cb0, kb1, n1, Lw, Ww, beta, what):
    """Launch the snapshot and the steps cb0 .. kb1 and judge what comes back.  Returns (L, W, worst ratio)."""
    npad = L0.shape[0]
    b0, nb = cb0 // RB, -(-n1 // RB) - cb0 // RB
    L, W, snap = gpm.remove_block_check(L0.reshape(-1), npad, W0, mw, cb0, kb1, n1, snap0, b0, nb)
    L, Wv = L.reshape(npad, npad), W[:mw * npad].reshape(mw, npad)
    done = min(kb1 + RB, n1)
    # what the launches must leave alone
    assert same_bits(L[~low], L0[~low]), "L was written left of the block, above the diagonal or from row n1 on"
    right = low.copy()
    right[:, :kb1 + RB] = False  # the columns right of the last step's block
    assert same_bits(L[right], L0[right]), "L was written right of column kb + 127"
    W0v = W0[:mw * npad].reshape(mw, npad)
    first = min(cb0 + RB, n1)  # the first block's rows stay as given; a later block's as the steps before it left them
    assert same_bits(Wv[:, :first], W0v[:, :first]), "the rows of W above kb, or the block's own, were written"
    assert same_bits(Wv[:, n1:], W0v[:, n1:]) and same_bits(W[mw * npad:], W0[mw * npad:]), "W was written from row n1 on"
    for b in range(npad // RB):
        blk = snap[b * RB * RB:(b + 1) * RB * RB].reshape(RB, RB)  # column-major
        if b0 <= b < b0 + nb:
            D = L0[b * RB:(b + 1) * RB, b * RB:(b + 1) * RB]
            assert same_bits(blk, np.ascontiguousarray(np.where(np.tril(np.ones((RB, RB), bool)), D, 0.0).T)), "snapshot %d" % b
        else:
            untouched(blk, "the snapshot of a block outside the launch")
    untouched(snap[npad * RB:], "the snapshot's tail")
    # the values: the orthogonal invariant within the bound of an fp64 evaluation, the elements within the cap
    live = low.copy()
    live[:, kb1 + RB:] = False
    assert np.isfinite(L[live]).all() and np.isfinite(Wv[:, cb0:n1]).all()
    Rs, B, gmax = R.remove_residual(Lt, Wp, np.where(live, L, 0.0), np.where(np.isfinite(Wv), Wv, 0.0), cb0, kb1, n1, beta)
    assert B.max() <= 1e-10 * gmax, "%s: the bound is too loose to judge by" % what
    err = np.abs(Rs).astype(np.float64)
    ratio = float((err / np.maximum(B, 1e-300)).max())
    assert (err <= B).all(), "%s: Z' Z'^T - Z Z^T outside the bound at %d places, worst |err| / e = %g" % (
        what, int((err > B).sum()), ratio)
    for got, want, name in ((L[live], Lw[live], "L"), (Wv[:, first:n1], Ww[:, first:n1], "W")):
        if got.size:
            d = float(np.abs(got.astype(np.longdouble) - want).max())
            cap = 1e-10 * float(np.abs(want).max())
            assert d <= cap, "%s: %s is %g from the long-double run (cap %g)" % (what, name, d, cap)
            ratio = max(ratio, d / max(cap, 1e-300))
    return L, W, ratio


def remove_id(c):
    return "n%d-mw%d-mc%d-cb%d%s" % (c[:4] + ("-single" if c[4] else "",))


@pytest.mark.parametrize("n1,mw,mc,cb0,single", R.REMOVE_CASES, ids=[remove_id(c) for c in R.REMOVE_CASES])
def test_remove_block(gpm, n1, mw, mc, cb0, single):
    Lt, Wp, Lw, Ww, beta = R.remove_problem(n1, mc, mw, cb0, single)
    assert not Wp[:, :cb0].any() and (single or not np.abs(Wp[:, :n1]).sum(0).all()), "no row of W with a zero top"
    kb1 = cb0 if single else (n1 - 1) // RB * RB
    L0, low, W0, snap0 = device_operands(Lt, Wp, cb0, n1)
    what = remove_id((n1, mw, mc, cb0, single))
    _, _, ratio = check_blocks(gpm, L0, low, W0, snap0, Lt, Wp, mw, cb0, kb1, n1, Lw, Ww, beta, what)
    print("RATIO remove_block %s %.4f" % (what, ratio))


def test_remove_two_passes(gpm):
    """m = 33: a pass of 32 columns, then one of a single column against the factor the first pass left."""
    n1, m = R.TWO_PASS
    Lt, W = R.remove_operands(n1, m)
    kb1 = (n1 - 1) // RB * RB
    W1 = np.ascontiguousarray(W[:32])
    W2 = np.zeros((32, Lt.shape[0]))
    W2[0] = W[32]
    L1w, W1w, beta1 = R.remove_blocks_ref(Lt, W1, 0, kb1, n1)
    L0, low, W0, snap0 = device_operands(Lt, W1, 0, n1)
    L1, _, r1 = check_blocks(gpm, L0, low, W0, snap0, Lt, W1, 32, 0, kb1, n1, L1w, W1w, beta1, "pass 1")
    # pass 2 starts from what the device left: its own invariant, the bound carried on from zero for these inputs
    L1t = np.where(low, L1, np.eye(Lt.shape[0]))
    L2w, W2w, beta2 = R.remove_blocks_ref(L1t, W2, 0, kb1, n1)
    _, low2, W0b, _ = device_operands(L1t, W2, 0, n1)
    _, _, r2 = check_blocks(gpm, L1, low2, W0b, snap0, L1t, W2, 32, 0, kb1, n1, L2w, W2w, beta2, "pass 2")
    print("RATIO remove_block two passes %.4f" % max(r1, r2))
