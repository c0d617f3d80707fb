"""The small kernels that finish a leave-one-out, multi-output or sparse evaluation, in isolation (run with -m gpu on the
MI355X box): loo_stats_kernel, loo_scale_symv_kernel + loo_u_final_kernel and loo_rank2_kernel (loo.hip), multi_dots_kernel
(multi.hip), and of sparse.hip the kernels finish_b, copy_upper, weights, scalars, sumsq, predict, multi_weights,
multi_dots, multi_sumsq, multi_pad and multi_sigma.

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h (gp.finish_check), which copy whole
host arrays to the device and back.  The three kinds of check of tests/test_update_kernels.py, with the references and the
accuracy model of tests/finish_kernels_ref.py:
- exact: integer / dyadic operands -- BIT FOR BIT, quotients and roots included where they are powers of two or perfect
  squares;
- full mantissa: random operands against the long-double evaluation of the same operations, |got - want| <= e (judge()
  asserts max(e) <= 1e-10 max |want|, so the bound cannot hide a failure);
- sentinels: NaNs with a payload in everything a launch must not read and everything it must not write; they come back bit
  for bit, and judge() fails on any non-finite result.
Every launch runs twice and must give the same bits; every test prints its worst |err| / e on a RATIO line.
"""
import numpy as np
import pytest

import finish_kernels_ref as R
from cases import NAN64
from test_substitution_kernels import judge, same_bits
from test_update_kernels import sentinels, untouched

pytestmark = pytest.mark.gpu
F64 = np.float64


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def launch(gpm, which, **args):
    """The hook twice on the same arguments: the same bits both times ("two identical calls give the same bits")."""
    a, b = gpm.finish_check(which, **args), gpm.finish_check(which, **args)
    several = isinstance(a, tuple)
    for x, y in zip(a if several else (a,), b if several else (b,)):
        assert same_bits(x, y), "%s: two identical launches differ in bits" % which
    return a


def zeros_exactly(a, what):
    """+0.0 everywhere, bit for bit."""
    a = np.ascontiguousarray(a)
    assert same_bits(a, np.zeros(a.shape)), "%s: not exact +0.0 everywhere" % what


# ---------------------------------------------------------------------------------------------------------------------
# loo.hip
# ---------------------------------------------------------------------------------------------------------------------
def run_stats(gpm, npad, n, kap, a, y):
    """loo_stats on sentinel-filled arrays; checks what must stay untouched and returns the launch's six outputs."""
    ld, nb = npad + 8, npad // 256
    out = launch(gpm, "loo_stats", Kinv=R.lower_flat(np.diag(kap), npad, ld, diag_only=True), ld=ld,
                 alpha=R.padded(a, (npad,)), y=R.padded(y, (npad,)), n=n, npad=npad, mu=sentinels(npad),
                 sigma=sentinels(npad), logp=sentinels(npad), v=sentinels(npad + 5), sc=sentinels(npad + 5),
                 part=sentinels(nb + 5))
    mu, sigma, logp, v, sc, part = out
    for x, name in ((mu, "mu"), (sigma, "sigma"), (logp, "logp")):
        untouched(x[n:], name + " from row n on")
    for x, name in ((v, "v"), (sc, "sc")):
        zeros_exactly(x[n:npad], name + " on n <= i < npad")  # the contract loo_scale_symv_kernel relies on
        untouched(x[npad:], name + " behind npad")
    untouched(part[nb:], "part behind the last block")
    return mu[:n], sigma[:n], logp[:n], v[:npad], sc[:npad], part[:nb]


@pytest.mark.parametrize("npad,n", R.STATS_CASES)
def test_loo_stats(gpm, npad, n):
    worst = 0.0
    for exact in (True, False):
        p = R.stats_problem(npad, n, exact)
        got = run_stats(gpm, npad, n, p["kap"], p["a"], p["y"])
        want, e = R.stats_ref(p["kap"], p["a"], p["y"], npad)
        names = ("mu", "sigma", "logp", "v", "sc", "part")
        for g, w, b, name in zip(got, want, e, names):
            bitwise = exact and name in ("mu", "sigma", "v")
            worst = max(worst, judge(g, w, None if bitwise else b, name))
        if n <= npad - 256:
            zeros_exactly(got[5][-1:], "the block sum of a block without a live row")
    print("RATIO loo_stats npad%d n%d %.4f" % (npad, n, worst))


def run_symv(gpm, npad, n, K, sc, v, exact, ref64=False):
    """loo_scale_symv on (K, sc, v); judges B and u and returns the worst ratio.  sc and v hold zeros from row n on: the
    launcher's stated precondition (the kernel multiplies the masked zeros of the rows and columns >= n by them)."""
    ld, ldb, nt = npad + 8, npad + 16, npad // 64
    assert not sc[n:].any() and not v[n:].any()
    B, upart, u = launch(gpm, "loo_scale_symv", Kinv=R.lower_flat(K, npad, ld), ld=ld, n=n, npad=npad, sc=sc, v=v,
                         B=sentinels((npad + 1) * ldb), ldb=ldb, upart=sentinels(nt * npad + 5), u=sentinels(npad + 5))
    if ref64:  # integer operands: the float64 evaluation is the exact one
        (Bw, uw), (eB, eu) = R.symv_eval(K, sc, v, npad, F64), (None, None)
    else:
        (Bw, uw), (eB, eu) = R.symv_ref(K, sc, v, npad)
    Bv = B.reshape(npad + 1, ldb)
    worst = judge(Bv[:npad, :npad], Bw, None if exact else eB, "B")
    zeros_exactly(Bv[n:npad, :npad], "B rows >= n")
    zeros_exactly(Bv[:npad, n:npad], "B columns >= n")
    untouched(Bv[:npad, npad:], "B columns >= npad")
    untouched(Bv[npad:], "B behind the last row")
    assert np.isfinite(upart[:nt * npad]).all(), "a (slot, row) of upart was not written (or holds a non-finite sum)"
    untouched(upart[nt * npad:], "upart behind the last slot")
    worst = max(worst, judge(u[:npad], uw, None if exact else eu, "u"))
    zeros_exactly(u[n:npad], "u from row n on")
    untouched(u[npad:], "u behind npad")
    return worst


@pytest.mark.parametrize("npad,n", R.SYMV_CASES + [R.SYMV_EXACT_ONLY])
def test_loo_scale_symv(gpm, npad, n):
    worst = 0.0
    for exact in ((True,) if (npad, n) == R.SYMV_EXACT_ONLY else (True, False)):
        p = R.symv_problem(npad, n, exact)
        worst = max(worst, run_symv(gpm, npad, n, p["K"], p["sc"], p["v"], exact, ref64=exact))
    print("RATIO loo_scale_symv npad%d n%d %.4f" % (npad, n, worst))


def test_loo_stats_feeds_scale_symv(gpm):
    """The v and sc that loo_stats writes into sentinel-filled arrays meet the precondition of loo_scale_symv: zeros from row
    n on.  The second launch is judged against the reference on the values the first one returned."""
    npad, n = 512, 300
    s, p = R.stats_problem(npad, n, False), R.symv_problem(npad, n, False)
    K = p["K"].copy()
    K[np.arange(n), np.arange(n)] = s["kap"]
    v, sc = run_stats(gpm, npad, n, s["kap"], s["a"], s["y"])[3:5]
    print("RATIO loo_stats->loo_scale_symv npad%d n%d %.4f" % (npad, n, run_symv(gpm, npad, n, K, sc, v, False)))


@pytest.mark.parametrize("npad,n", R.RANK2_CASES)
def test_loo_rank2(gpm, npad, n):
    ld, lt = npad + 8, R.lower_tiles(npad)
    worst = 0.0
    for exact in (True, False):
        p = R.rank2_problem(npad, n, exact)
        G0 = sentinels((npad + 1) * ld)
        G0v = G0.reshape(npad + 1, ld)[:npad, :npad]
        G0v[lt] = p["G"][lt]  # finite on the lower 64-tiles (whole diagonal tiles), sentinels strictly above them
        G = launch(gpm, "loo_rank2", G=G0, ld=ld, n=n, npad=npad, u=p["u"], alpha=R.padded(p["alpha"], (npad,)))
        Gv = G.reshape(npad + 1, ld)
        untouched(Gv[:npad, :npad][~lt], "G on the tiles strictly above the diagonal")
        untouched(Gv[:npad, npad:], "G columns >= npad")
        untouched(Gv[npad:], "G behind the last row")
        want, e = R.rank2_ref(p["G"], p["u"], p["alpha"])
        live = lt[:n, :n]
        worst = max(worst, judge(Gv[:n, :n][live], want[live], None if exact else e[live], "G"))
        keep = lt.copy()
        keep[:n, :n] = False
        assert same_bits(Gv[:npad, :npad][keep], p["G"][keep]), "an element with i >= n or j >= n changed its bits"
    print("RATIO loo_rank2 npad%d n%d %.4f" % (npad, n, worst))


# ---------------------------------------------------------------------------------------------------------------------
# the sums of products: multi_dots, sparse_sumsq, sparse_multi_sumsq, sparse_multi_dots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", R.DOTS_CASES)
def test_multi_dots(gpm, n, T):
    ld = R.up256(n)
    worst = 0.0
    for exact in (True, False):
        p = R.dots_problem(1, T, n, exact)
        dots = launch(gpm, "multi_dots", Yt=R.padded(p["A"], (T + 1, ld)), At=R.padded(p["B"], (T + 1, ld)), ld=ld, n=n, T=T,
                      dots=sentinels(T + 5))
        want, e = R.dots_ref(p["A"], p["B"])
        worst = max(worst, judge(dots[:T], want, None if exact else e, "dots"))
        untouched(dots[T:], "dots behind T")
    print("RATIO multi_dots n%d T%d %.4f" % (n, T, worst))


@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sparse_sumsq(gpm, n):
    worst = 0.0
    for exact in (True, False):
        y = R.dots_problem(2, 1, n, exact)["A"]
        out = launch(gpm, "sparse_sumsq", y=R.padded(y, (1, n + 7)), n=n, out=sentinels(4))
        want, e = R.dots_ref(y, y)
        worst = max(worst, judge(out[:1], want, None if exact else e, "sum y^2"))
        untouched(out[1:], "out behind the sum")
    print("RATIO sparse_sumsq n%d %.4f" % (n, worst))


@pytest.mark.parametrize("T", R.SUMSQ_T)
@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_sparse_multi_sumsq(gpm, n, T):
    ldy = T + 3
    worst = 0.0
    for exact in (True, False):
        Yt = R.dots_problem(3, T, n, exact)["A"]
        out = launch(gpm, "sparse_multi_sumsq", Y=R.padded(np.ascontiguousarray(Yt.T), (n + 1, ldy)), ldy=ldy, n=n, T=T,
                     out=sentinels(T + 3))
        want, e = R.dots_ref(Yt, Yt)
        worst = max(worst, judge(out[:T], want, None if exact else e, "sum Y^2"))
        untouched(out[T:], "out behind T")
    print("RATIO sparse_multi_sumsq n%d T%d %.4f" % (n, T, worst))


@pytest.mark.parametrize("M,T", R.MDOTS_CASES)
def test_sparse_multi_dots(gpm, M, T):
    ld, ts = M + 9, T + 2
    worst = 0.0
    for exact in (True, False):
        p = R.dots_problem(4, T, M, exact)
        out = launch(gpm, "sparse_multi_dots", Rt=R.padded(p["A"], (T + 1, ld)), Gt=R.padded(p["B"], (T + 1, ld)), ld=ld, M=M,
                     T=T, tstride=ts, out=sentinels(2 * ts + 3))
        for o, (want, e), name in ((0, R.dots_ref(p["A"], p["B"]), "r . gamma"), (ts, R.dots_ref(p["B"], p["B"]), "gamma^2")):
            worst = max(worst, judge(out[o:o + T], want, None if exact else e, name))
        untouched(out[T:ts], "out[T .. tstride)")
        untouched(out[ts + T:], "out behind tstride + T")
    print("RATIO sparse_multi_dots M%d T%d %.4f" % (M, T, worst))


# ---------------------------------------------------------------------------------------------------------------------
# the Mp x Mp element-wise kernels
# ---------------------------------------------------------------------------------------------------------------------
def check_square(out, Mp, want, e, what):
    r = judge(out[:Mp * Mp].reshape(Mp, Mp), want, e, what)
    untouched(out[Mp * Mp:], what + " behind Mp^2")
    return r


@pytest.mark.parametrize("Mp", R.MPS)
def test_sparse_finish_b(gpm, Mp):
    worst = 0.0
    for exact in (True, False):
        Bacc = R.square_problem(1, Mp, exact)["B"]
        seen = Bacc.copy()
        seen[np.triu_indices(Mp, 1)] = NAN64  # only a >= b is read
        inv_s2 = R.S4_DYADIC if exact else R.S4_PLAIN
        B = launch(gpm, "sparse_finish_b", Bacc=R.with_tail(seen), Mp=Mp, inv_s2=inv_s2, B=sentinels(Mp * Mp + 5))
        want, e = R.finish_b_ref(Bacc, inv_s2)
        worst = max(worst, check_square(B, Mp, want, None if exact else e, "B"))
        Bv = B[:Mp * Mp].reshape(Mp, Mp)
        assert same_bits(Bv, np.ascontiguousarray(Bv.T)), "B and its transpose differ in bits"
    print("RATIO sparse_finish_b Mp%d %.4f" % (Mp, worst))


@pytest.mark.parametrize("Mp", R.MPS)
def test_sparse_copy_upper(gpm, Mp):
    src = R.square_problem(2, Mp, False)["B"].copy()
    src[0, :3] = [-0.0, 5e-324, 1.0]  # a copy keeps the sign of a zero and a denormal
    want = np.triu(src)
    want[np.tril_indices(Mp, -1)] = 0.0
    src[np.tril_indices(Mp, -1)] = NAN64
    dst = launch(gpm, "sparse_copy_upper", src=R.with_tail(src), Mp=Mp, dst=sentinels(Mp * Mp + 5))
    assert same_bits(dst[:Mp * Mp].reshape(Mp, Mp), want), "not a bit-for-bit copy on j >= i with +0.0 below"
    untouched(dst[Mp * Mp:], "dst behind Mp^2")
    print("RATIO sparse_copy_upper Mp%d 0.0000 (bit for bit)" % Mp)


@pytest.mark.parametrize("Mp", R.MPS)
def test_sparse_weights(gpm, Mp):
    worst = 0.0
    for exact in (True, False):
        p = R.square_problem(3, Mp, exact)
        s4 = R.S4_DYADIC if exact else R.S4_PLAIN
        T, S = launch(gpm, "sparse_weights", B=R.with_tail(p["B"]), Binv=R.with_tail(p["Binv"]), g=R.with_tail(p["g"]), Mp=Mp,
                      s4=s4, T=sentinels(Mp * Mp + 5), S=sentinels(Mp * Mp + 5))
        (Tw, Sw), (eT, eS) = R.weights_ref(p["B"], p["Binv"], p["g"], s4)
        worst = max(worst, check_square(T, Mp, Tw, None if exact else eT, "T"),
                    check_square(S, Mp, Sw, None if exact else eS, "S"))
    print("RATIO sparse_weights Mp%d %.4f" % (Mp, worst))


@pytest.mark.parametrize("nT", R.NTS)
@pytest.mark.parametrize("Mp", R.MPS)
def test_sparse_multi_weights(gpm, Mp, nT):
    worst = 0.0
    for exact in (True, False):
        p = R.square_problem(4, Mp, exact)
        s4 = R.S4_DYADIC if exact else R.S4_PLAIN
        Tm, S = launch(gpm, "sparse_multi_weights", B=R.with_tail(p["B"]), Binv=R.with_tail(p["Binv"]), GG=R.with_tail(p["GG"]),
                       Mp=Mp, T=nT, s4=s4, Tm=sentinels(Mp * Mp + 5), S=sentinels(Mp * Mp + 5))
        (Tw, Sw), (eT, eS) = R.multi_weights_ref(p["B"], p["Binv"], p["GG"], nT, s4)
        worst = max(worst, check_square(Tm, Mp, Tw, None if exact else eT, "Tm"),
                    check_square(S, Mp, Sw, None if exact else eS, "S"))
    print("RATIO sparse_multi_weights Mp%d T%d %.4f" % (Mp, nT, worst))


@pytest.mark.parametrize("M", R.SCALARS_M)
def test_sparse_scalars(gpm, M):
    Mp = R.SCALARS_MP
    worst = 0.0
    for exact in (True, False):
        p = R.scalars_problem(M, exact)
        diag = lambda d: R.lower_flat(np.diag(d), Mp, Mp, diag_only=True)  # noqa: E731
        out = launch(gpm, "sparse_scalars", C=diag(p["c"]), B=diag(p["b"]), Binv=diag(p["bi"]), r=R.padded(p["r"], (Mp,)),
                     g=R.padded(p["g"], (Mp,)), M=M, Mp=Mp, out=sentinels(8))
        want, e = R.scalars_ref(p["c"], p["b"], p["bi"], p["r"], p["g"])
        worst = max(worst, judge(out[:1], want[:1], e[:1], "sum 2 log C_ii"))
        worst = max(worst, judge(out[1:5], want[1:], None if exact else e[1:], "out[1 .. 4]"))
        untouched(out[5:], "out[5 ..]")
    print("RATIO sparse_scalars M%d %.4f" % (M, worst))


# ---------------------------------------------------------------------------------------------------------------------
# sparse_multi_pad, sparse_predict, sparse_multi_sigma
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,kp,rpad", R.PAD_CASES)
def test_sparse_multi_pad(gpm, rows, T, kp, rpad):
    ldy, ldp = T + 3, kp + 8
    Y = R.dots_problem(5, rows, T, False)["A"].copy()
    Y[0, 0] = -0.0
    Yp = launch(gpm, "sparse_multi_pad", Y=R.padded(Y, (rows + 1, ldy)), ldy=ldy, rows=rows, T=T, kp=kp, rpad=rpad,
                Yp=sentinels((rpad + 1) * ldp), ldp=ldp).reshape(rpad + 1, ldp)
    want = np.zeros((rpad, kp))
    want[:rows, :T] = Y
    assert same_bits(np.ascontiguousarray(Yp[:rpad, :kp]), want), "not the rows of Y, bit for bit, with +0.0 around them"
    untouched(Yp[:rpad, kp:], "Yp columns >= kp")
    untouched(Yp[rpad:], "Yp behind rpad rows")
    print("RATIO sparse_multi_pad rows%d T%d kp%d rpad%d 0.0000 (bit for bit)" % (rows, T, kp, rpad))


@pytest.mark.parametrize("m,ncols", R.PREDICT_CASES)
def test_sparse_predict_and_multi_sigma(gpm, m, ncols):
    ld = R.PREDICT_LD
    worst = 0.0
    for exact in (True, False):
        p = R.predict_problem(m, ncols, exact)
        (muw, sw), (emu, es) = R.predict_ref(p["A"], p["V"], p["prior"], p["q"], p["dot"], p["inv_s2"])
        shared = dict(A=R.padded(p["A"], (m + 1, ld)), V=R.padded(p["V"], (m + 1, ld)), ld=ld, ncols=ncols, m=m,
                      prior=R.padded(p["prior"], (m + 3,)), q=R.padded(p["q"], (m + 3,)))
        mu, sigma = launch(gpm, "sparse_predict", dot=R.padded(p["dot"], (m + 3,)), inv_s2=p["inv_s2"], mu=sentinels(m + 3),
                           sigma=sentinels(m + 3), **shared)
        sigma2 = launch(gpm, "sparse_multi_sigma", sigma=sentinels(m + 3), **shared)
        worst = max(worst, judge(mu[:m], muw, None if exact else emu, "mu"))
        for s, name in ((sigma, "sigma of predict"), (sigma2, "sigma of multi_sigma")):
            worst = max(worst, judge(s[:m], sw, None if exact else es, name))
            untouched(s[m:], name + " from m on")
        untouched(mu[m:], "mu from m on")
    print("RATIO sparse_predict/multi_sigma m%d ncols%d %.4f" % (m, ncols, worst))
