"""The kernels that consume the factor, in isolation (run with -m gpu on the MI355X box): the one-pass substitution of
trsm_small.hip (every instance, double and float), and of solve.hip the substitution steps, alpha_from_y, rownorm_dot,
tinv_init and the batched 256-block product blockmm.

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h, which copy whole host arrays to
the device and back.  Three kinds of check (tests/substitution_ref.py holds the references):
- exact: integer operands ({-1, 0, 1} matrices, right-hand sides in [-8, 8]; dyadic m / 2^20 for the plain products)
  whose partial sums stay below 2^53 in any order -- the fp64 arithmetic of every kernel here (the float instances too:
  only their matrices are float) must return the integer reference BIT FOR BIT;
- full mantissa: random operands against a long-double run of the same recurrence, |V - V_ref| <= e with the running
  bound e of an fp64 evaluation in any order -- small integers have a zero low word and cannot see the granule
  packing, the float widening or a narrowed accumulate; these can.  For the float instances the operands are rounded
  to float first: the arithmetic is fp64 either way, so the same bound holds.  max(e) <= 1e-10 max |V| is asserted, so
  the bound cannot hide a failure;
- sentinels: NaNs with a payload in everything a launch must not read (the diagonal blocks of L and all to their right,
  the padding columns, the rows of KsT an instance does not address) or write (they come back bit for bit).

A non-zero time-out word of the one-pass kernel fails the test with the code printed; nothing here waits for one.
"""
import numpy as np
import pytest

import substitution_ref as R
from cases import NAN32, NAN64
from test_tile_kernels import dyadic

pytestmark = pytest.mark.gpu

P = R.P
U = R.U


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def dtype_of(prec):
    return np.float64 if prec == 64 else np.float32


def nan_of(dt):
    return NAN64 if dt == np.float64 else NAN32


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def flat_factor(L, ld, dt, out=None, off=0):
    """The factor as the launches see it: leading dimension ld, sentinels on the diagonal blocks, right of them and in
    the padding columns -- only the blocks strictly below the diagonal hold data."""
    npad = L.shape[0]
    if out is None:
        out = np.full(npad * ld, nan_of(dt), dt)
    v = out[off:off + npad * ld].reshape(npad, ld)
    for B in range(1, npad // P):
        v[B * P:(B + 1) * P, :B * P] = L[B * P:(B + 1) * P, :B * P]
    return out


def problem(data, npad, prec, **kw):
    """(L, Dinv, b, V, W, E, EW) of the shared problem; E = EW = None for the exact one."""
    if data == "exact":
        return R.exact_problem(npad, **kw) + (None, None)
    return R.mantissa_problem(npad, prec == 32, **kw)


def judge(got, want, bound, what):
    """Bit equality with the integer reference, or |got - want| <= bound.  Returns the largest |got - want| / bound."""
    assert np.isfinite(got).all(), "%s: %d non-finite values" % (what, int((~np.isfinite(got)).sum()))
    if bound is None:
        bad = np.argwhere(got != want.astype(np.float64))
        assert bad.size == 0, "%s: %d of %d differ, first at %s: %r vs %r" % (
            what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        return 0.0
    assert bound.max() <= 1e-10 * float(np.abs(want).max()), "%s: the bound is too loose to judge by" % what
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), "%s: %d of %d outside the bound, worst |err| / e = %g" % (
        what, int((err > bound).sum()), got.size, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# the one-pass substitution
# ---------------------------------------------------------------------------------------------------------------------
TRSM64 = [(0, 1), (32, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 8), (0, 9), (0, 16), (0, 17), (0, 32), (32, 32)]
TRSM32 = [(0, 1), (0, 2), (0, 4), (0, 7), (0, 16), (0, 32)]
TRSM_CASES = [(p, npad, j0, cnt, data)
              for p, lst in ((64, TRSM64), (32, TRSM32)) for (j0, cnt) in lst for npad in R.NPADS
              for data in ("exact", "mantissa")]
TRSM_CASES += [(64, R.NPAD_BIG, 0, 1, "mantissa"), (64, R.NPAD_BIG, 0, 17, "mantissa")]


def trsm_id(c):
    p, npad, j0, cnt, data = c
    return "f%d-%s-j%d-c%d-n%d-%s" % (p, R.expected_solution(p, j0, cnt)[0], j0, cnt, npad, data)


def test_every_instance_is_named():
    names = {trsm_id(c).split("-j")[0] for c in TRSM_CASES}
    assert names == {"f64-granule"} | {"f%d-NT1-MC%d" % (p, mc) for p in (64, 32) for mc in (1, 2, 4, 8, 16)} | {
        "f64-NT2-MC32", "f32-NT2-MC32"}, sorted(names)


@pytest.mark.parametrize("prec,npad,j0,cnt,data", TRSM_CASES, ids=[trsm_id(c) for c in TRSM_CASES])
def test_trsm_small(gpm, prec, npad, j0, cnt, data):
    dt = dtype_of(prec)
    name, kind, width = R.expected_solution(prec, j0, cnt)
    L, Dinv, b, V, _, E, _ = problem(data, npad, prec)
    ld = ldk = npad + 8
    Lf = flat_factor(L, ld, dt)
    Df = Dinv.astype(dt).reshape(-1)
    assert not np.triu(Dinv, 1).any()
    mp = 1 if name == "granule" else (16 if cnt <= 16 else 32)  # rows of KsT the instance reads, from j0 on
    K = np.full((j0 + mp + 2) * ldk, nan_of(dt), dt)
    Kv = K.reshape(-1, ldk)
    Kv[j0:j0 + cnt, :npad] = b[:, j0:j0 + cnt].T
    rng = np.random.default_rng(99 + npad + cnt)
    if mp > cnt:  # the padded right-hand sides: finite, from another seed
        fill = rng.integers(-8, 9, (mp - cnt, npad)) if data == "exact" else rng.standard_normal((mp - cnt, npad))
        Kv[j0 + cnt:j0 + mp, :npad] = fill
    assert np.array_equal(Kv[j0:j0 + cnt, :npad].astype(np.float64), b[:, j0:j0 + cnt].T)  # floats hold them exactly
    dq0 = np.full(j0 + cnt + 3, NAN64)
    ws0 = np.full(gpm.trsm_small_workspace(npad) // 8, NAN64).view(np.uint8)  # the launcher clears what it polls

    def launch(Kmat, ws):
        dq, ws, k, wd, off, tmo = gpm.trsm_small_check(npad, Lf, ld, Df, Kmat, ldk, j0, cnt, dq0, ws)
        assert tmo == 0, "a workgroup gave up waiting: time-out word 0x%x" % tmo
        assert (k, wd) == (kind, width), "trsm_small_solution reports kind %d width %d for the %s launch" % (k, wd, name)
        assert 0 <= off and off + npad * width * (16 if kind == R.TS_SOL_GRANULE else 8) <= ws.size
        return dq, ws, R.decode_solution(ws, k, wd, off, npad)

    dq, ws, Vg = launch(K, ws0)
    ratio = judge(Vg[:, :cnt], V[:, j0:j0 + cnt], None if E is None else E[:, j0:j0 + cnt], "V")
    print("RATIO f%d-%s n%d %s %.4f" % (prec, name, npad, data, ratio))
    # |V_j|^2: sums of non-negative terms
    ref = R.sumsq_exact(V[:, j0:j0 + cnt]) if data == "exact" else (
        (V[:, j0:j0 + cnt] * V[:, j0:j0 + cnt]).sum(0).astype(np.float64))
    assert (np.abs(dq[j0:j0 + cnt] - ref) <= (npad + 4) * U * ref).all(), (dq[j0:j0 + cnt], ref)
    outside = np.r_[0:j0, j0 + cnt:dq.size]
    assert same_bits(dq[outside], dq0[outside]), "dq was written outside [j0, j0 + cnt)"
    # again, on the workspace the first launch left behind (its counters, tags and solution): bit for bit
    dq2, ws2, Vg2 = launch(K, ws)
    assert same_bits(Vg2[:, :cnt], Vg[:, :cnt]) and same_bits(dq2, dq)
    if mp > cnt:  # ... and the padded right-hand sides change nothing: zeros there give the same bits
        K0 = K.copy()
        K0.reshape(-1, ldk)[j0 + cnt:j0 + mp, :npad] = 0
        dq3, _, Vg3 = launch(K0, ws0)
        assert same_bits(Vg3[:, :cnt], Vg[:, :cnt]) and same_bits(dq3, dq)


# ---------------------------------------------------------------------------------------------------------------------
# the substitution steps of solve.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["exact", "mantissa"])
@pytest.mark.parametrize("npad", [256, 768, 1280])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("prec", [64, 32], ids=["f64", "f32"])
def test_trsv_whole_chain(gpm, prec, direction, npad, data):
    dt = dtype_of(prec)
    kw = dict(backward=True) if direction == "bwd" else {}
    L, Dinv, b, V, W, E, EW = problem(data, npad, prec, **kw)
    ld, nb = npad + 8, npad // P
    Lf, Df = flat_factor(L, ld, dt), Dinv.astype(dt).reshape(-1)
    w0, out0 = np.full(npad + 6, NAN64), np.full(npad + 6, NAN64)
    w0[:npad] = b[:, 0]
    w, out = gpm.trsv_steps_check(direction, npad, Lf, ld, Df, 0, nb - 1, w0, out0)
    col = lambda a: None if a is None else a[:, :1]  # noqa: E731
    ratio = judge(out[:npad, None], V[:, :1], col(E), "solution")
    judge(w[:npad, None], W[:, :1], col(EW), "w")  # every block of w ends as the w_B its own step consumed
    print("RATIO trsv-%s-f%d n%d %s %.4f" % (direction, prec, npad, data, ratio))
    assert same_bits(w[npad:], w0[npad:]) and same_bits(out[npad:], out0[npad:])


@pytest.mark.parametrize("data", ["exact", "mantissa"])
@pytest.mark.parametrize("npad", [768, 1280])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("prec", [64, 32], ids=["f64", "f32"])
def test_trsv_single_middle_step(gpm, prec, direction, npad, data):
    """Step b0 = b1 = 1 alone: which rows a step may touch."""
    dt = dtype_of(prec)
    L, Dinv, _, _, _, _, _ = problem(data, npad, prec)
    ld = npad + 8
    Lf, Df = flat_factor(L, ld, dt), Dinv.astype(dt).reshape(-1)
    rng = np.random.default_rng(31 + npad)
    w0, out0 = np.full(npad + 6, NAN64), np.full(npad + 6, NAN64)
    w0[:npad] = rng.integers(-8, 9, npad) if data == "exact" else rng.standard_normal(npad)
    w, out = gpm.trsv_steps_check(direction, npad, Lf, ld, Df, 1, 1, w0, out0)
    step = R.fwd_step if direction == "fwd" else R.bwd_step
    touched = slice(2 * P, npad) if direction == "fwd" else slice(0, P)
    if data == "exact":
        z, wn = step(L, Dinv, 1, w0[:npad], "int")
        judge(out[P:2 * P], z, None, "step solution")
        judge(w[touched], wn[touched], None, "updated w")
    else:
        z, wn, ez, ew = step(L, Dinv, 1, w0[:npad])
        judge(out[P:2 * P], z, ez, "step solution")
        judge(w[touched], wn[touched], ew[touched], "updated w")
    keep = np.ones(npad + 6, bool)
    keep[touched] = False
    assert same_bits(w[keep], w0[keep]), "the step wrote rows of w that are not its own"
    keep = np.ones(npad + 6, bool)
    keep[P:2 * P] = False
    assert same_bits(out[keep], out0[keep]), "the step wrote outside its block of the solution"


@pytest.mark.parametrize("data", ["exact", "mantissa"])
def test_trsv_forward_candidates(gpm, data):
    """Forward fp64, k = 3 candidates (tl_batch) with sentinel gaps between them."""
    npad, k = 768, 3
    ld, nb = npad + 8, npad // P
    bstride = npad * ld + 1024
    Lf = np.full((k - 1) * bstride + npad * ld, NAN64)
    Df = np.full((k - 1) * bstride + npad * P, NAN64)
    w0 = np.full((k - 1) * bstride + npad, NAN64)
    out0 = w0.copy()
    refs = []
    for c in range(k):
        if data == "exact":
            pr = R.exact_problem(npad, m=1, seed=5900 + c) + (None, None)
        else:
            pr = R.mantissa_problem(npad, False, m=1, seed=7900 + c)
        L, Dinv, b = pr[:3]
        flat_factor(L, ld, np.float64, Lf, c * bstride)
        Df[c * bstride:c * bstride + npad * P] = Dinv.reshape(-1)
        w0[c * bstride:c * bstride + npad] = b[:, 0]
        refs.append(pr)
    w, out = gpm.trsv_steps_check("fwd", npad, Lf, ld, Df, 0, nb - 1, w0, out0, k=k, bstride=bstride)
    gap = np.ones(w0.size, bool)
    for c, (L, Dinv, b, V, W, E, EW) in enumerate(refs):
        sl = slice(c * bstride, c * bstride + npad)
        gap[sl] = False
        judge(out[sl, None], V, E, "candidate %d" % c)
        judge(w[sl, None], W, EW, "w of candidate %d" % c)
    assert same_bits(w[gap], w0[gap]) and same_bits(out[gap], out0[gap])


# ---------------------------------------------------------------------------------------------------------------------
# the small consumers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["exact", "mantissa"])
@pytest.mark.parametrize("npad", [256, 768])
@pytest.mark.parametrize("prec", [64, 32], ids=["f64", "f32"])
def test_alpha_from_y(gpm, prec, npad, data):
    """alpha_i = sum_{q >= q0(i)} Y[i][q] z[q]: the block-lower part of Y left of each row's 256-block holds NaN."""
    dt = dtype_of(prec)
    rng = np.random.default_rng(41 + npad)
    ld = npad + 8
    Y = np.full((npad, ld), nan_of(dt), dt)
    Yd = np.zeros((npad, npad))
    for B in range(npad // P):
        blk = dyadic(rng, (P, npad - B * P)) if data == "exact" else rng.standard_normal((P, npad - B * P))
        Y[B * P:(B + 1) * P, B * P:npad] = blk
        Yd[B * P:(B + 1) * P, B * P:] = Y[B * P:(B + 1) * P, B * P:npad]
    z = np.full(npad + 4, NAN64)
    z[:npad] = dyadic(rng, npad) if data == "exact" else rng.standard_normal(npad)
    a0 = np.full(npad + 4, NAN64)
    a = gpm.alpha_from_y_check(npad, Y.reshape(-1), ld, z, a0)
    assert same_bits(a[npad:], a0[npad:])
    if data == "exact":  # products m m' / 2^40, up to 768 of them: below 2^53 units in any order
        assert np.array_equal(a[:npad], Yd @ z[:npad])
    else:
        want = Yd.astype(np.longdouble) @ z[:npad].astype(np.longdouble)
        bound = R.gamma(npad + 1) * (np.abs(Yd) @ np.abs(z[:npad]))
        assert (np.abs(a[:npad].astype(np.longdouble) - want).astype(np.float64) <= bound).all()


@pytest.mark.parametrize("null", ["none", "vec", "dot", "sq", "vec+dot"])
@pytest.mark.parametrize("data", ["exact", "mantissa"])
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("prec", [64, 32], ids=["f64", "f32"])
def test_rownorm_dot(gpm, prec, m, data, null):
    dt = dtype_of(prec)
    ncols, ld = 600, 611  # not a multiple of 256; an odd leading dimension
    rng = np.random.default_rng(51 + m)
    V = np.full((m + 1, ld), nan_of(dt), dt)
    V[:m, :ncols] = dyadic(rng, (m, ncols)) if data == "exact" else rng.standard_normal((m, ncols))
    Vd = V[:m, :ncols].astype(np.float64)
    vec = None if "vec" in null else np.r_[dyadic(rng, ncols) if data == "exact" else rng.standard_normal(ncols),
                                           [NAN64] * 3]
    dot0 = None if "dot" in null else np.full(m + 2, NAN64)
    sq0 = None if "sq" in null else np.full(m + 2, NAN64)
    dot, sq = gpm.rownorm_dot_check(V.reshape(-1), ld, ncols, m, vec, dot0, sq0)
    vv = np.zeros(ncols) if vec is None else vec[:ncols]  # no vector: the dot is the empty sum
    for got, before, want, mag in ((dot, dot0, Vd.astype(np.longdouble) @ vv.astype(np.longdouble), np.abs(Vd) @ np.abs(vv)),
                                   (sq, sq0, (Vd.astype(np.longdouble) ** 2).sum(1), (Vd ** 2).sum(1))):
        if before is None:
            assert got is None
            continue
        assert same_bits(got[m:], before[m:])
        if data == "exact":
            assert np.array_equal(got[:m], want.astype(np.float64))
        else:
            assert (np.abs(got[:m].astype(np.longdouble) - want).astype(np.float64) <= R.gamma(ncols + 1) * mag).all()


# ---------------------------------------------------------------------------------------------------------------------
# the T^-1 assembly
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_xt", [False, True], ids=["X", "X+XT"])
@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("prec", [64, 32], ids=["f64", "f32"])
def test_tinv_init(gpm, prec, nsub, with_xt):
    dt = dtype_of(prec)
    n, tld = nsub * P, nsub * P + 8
    rng = np.random.default_rng(61 + nsub)
    Dinv = rng.standard_normal((nsub, P, P)).astype(dt)
    X0 = np.full(n * tld + 5, nan_of(dt), dt)
    X, XT = gpm.tinv_check(nsub, Dinv.reshape(-1), X0, tld, X0.copy() if with_xt else None)
    for got, transposed in ((X, False), (XT, True)):
        if got is None:
            assert not with_xt and transposed
            continue
        want = X0.copy()
        wv = want[:n * tld].reshape(n, tld)
        for i in range(nsub):
            for j in range(nsub):
                r, c = slice(i * P, (i + 1) * P), slice(j * P, (j + 1) * P)
                if i == j:
                    wv[r, c] = Dinv[i].T if transposed else Dinv[i]
                elif (i > j) if transposed else (i < j):
                    wv[r, c] = 0
        assert same_bits(got, want), "%d elements differ" % int((bits(got) != bits(want)).sum())


def blockmm_arena(rng, dt, Ks, k, data):
    """One arena per candidate: per product [A | gap | B | gap | C | gap], distinct leading dimensions, NaN gaps and C."""
    prods, off = [], 16
    for i, K in enumerate(Ks):
        lda, ldb, ldc = K + 8 * (i + 1), P + 8 * (i + 2), P + 8 * (i + 3)
        a_off = off
        b_off = a_off + P * lda + 24
        c_off = b_off + K * ldb + 40
        off = c_off + P * ldc + 56
        prods.append((a_off, lda, b_off, ldb, c_off, ldc, K))
    bstride = off + 64
    arena = np.full(bstride * k, nan_of(dt), dt)
    for c in range(k):
        for a_off, lda, b_off, ldb, c_off, ldc, K in prods:
            for o, rows, cols, ldx in ((a_off, P, K, lda), (b_off, K, P, ldb)):
                v = arena[c * bstride + o:c * bstride + o + rows * ldx].reshape(rows, ldx)
                if data == "dyadic":
                    v[:, :cols] = dyadic(rng, (rows, cols))
                elif data == "int":
                    v[:, :cols] = rng.integers(-8, 9, (rows, cols))
                else:
                    v[:, :cols] = rng.standard_normal((rows, cols))
    return arena, prods, bstride


K1, K6 = (256,), (32, 256, 768, 32, 768, 256)
BLOCKMM = [(64, "dyadic", K1, 1), (64, "dyadic", K6, 1), (64, "dyadic", (768, 32), 2),
           (32, "int", K1, 1), (32, "int", K6, 1), (32, "normal", K1, 1), (32, "normal", K6, 1)]


@pytest.mark.parametrize("alpha", [1.0, -1.0])
@pytest.mark.parametrize("prec,data,Ks,k", BLOCKMM,
                         ids=["f%d-%s-nprod%d-k%d" % (p, {"dyadic": "exact", "int": "exact", "normal": "bound"}[d], len(K), k)
                              for p, d, K, k in BLOCKMM])
def test_blockmm(gpm, prec, data, Ks, k, alpha):
    """C_b = alpha A_b B_b, plain A B.  fp64: dyadic operands m / 2^20, every partial sum below 2^53 units -- bit for bit.
    float: the arithmetic is fp64, so float inputs give an fp64-exact product (small integers: exactly; random: to
    K 2^-53, far below) which is rounded to float ONCE: |C - ref| <= (K + 4) 2^-24 |alpha| |A||B| bounds that rounding."""
    dt = dtype_of(prec)
    arena, prods, bstride = blockmm_arena(np.random.default_rng(71 + len(Ks)), dt, Ks, k, data)
    got = gpm.blockmm_check(arena, prods, alpha, k=k, bstride=bstride if k > 1 else 0)
    want = arena.copy()
    wrote = np.zeros(arena.size, bool)
    for c in range(k):
        for a_off, lda, b_off, ldb, c_off, ldc, K in prods:
            A = arena[c * bstride + a_off:][:P * lda].reshape(P, lda)[:, :K].astype(np.float64)
            B = arena[c * bstride + b_off:][:K * ldb].reshape(K, ldb)[:, :P].astype(np.float64)
            ref = alpha * (A @ B)
            Cg = got[c * bstride + c_off:][:P * ldc].reshape(P, ldc)[:, :P].astype(np.float64)
            wrote[c * bstride + c_off:][:P * ldc].reshape(P, ldc)[:, :P] = True
            if data == "normal":
                bound = (K + 4) * 2.0 ** -24 * (np.abs(A) @ np.abs(B))
                assert (np.abs(Cg - ref) <= bound).all(), (np.abs(Cg - ref) / bound).max()
            else:
                assert np.abs(A).max() * np.abs(B).max() * K < (2.0 ** 13 if data == "dyadic" else 2.0 ** 24)
                bad = np.argwhere(Cg != ref)
                assert bad.size == 0, "%d elements differ, first at %s" % (len(bad), tuple(bad[0]))
    assert same_bits(got[~wrote], want[~wrote]), "the launch wrote outside its C blocks"
