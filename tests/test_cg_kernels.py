"""The kernels of cg.hip in isolation (run with -m gpu on the MI355X box): kmm_kernel + kmm_finish_kernel (the matrix-free
multi-right-hand-side product on v_mfma_f64_16x16x4_f64), cg_dots_kernel + cg_dots_final_kernel with the per-column
decisions, cg_update_xr_kernel, cg_update_p_kernel, cg_scale_kernel, cg_status_kernel and the preconditioner's kernels
(cg_capacitance_kernel, cg_lst_kernel, cg_small_mm_kernel, cg_precond_kernel), all through the PRODUCT launchers via the
hooks of include/gogp_testhooks.h.  tests/cg_ref.py and tests/gram_ref.py hold the references and the bound's model.

- exact mode: inv_len = 0, dyadic c, integer V and integer diagonal -- the output and every slab partial are the integer
  product BIT FOR BIT (the partials against the restated slab model), at slab counts 1, 3 and 8 and with a block cap that
  makes a workgroup walk several tiles;
- long-double mode: |got - ref| <= gamma_n sum_j |K_ij V_tj| + sum_j e_ij |V_tj| element by element, the bound from the
  model and the inputs alone; the worst |err| / bound per family is printed by the last test (-s shows it);
- sentinels (payload NaNs) on everything a launch must not read or write: the rows of A / B from rows / cols on, V's
  columns from cols on and its rows from T on, the output's tails;
- the column-wise kernels on integers: exact bits; a frozen column keeps its bits.
Every launch runs twice and must return the same bits."""
import numpy as np
import pytest

import cg_ref as C
import gram_ref as R
from cases import NAN64

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
RATIOS = {}
EXACT_SHAPES = [(1, 1, 1, False), (63, 65, 1, False), (64, 64, 16, False), (100, 257, 17, False), (257, 100, 64, False),
                (193, 193, 33, True)]
LD_DIMS = (1, 3, 8, 17, 64)
LD_CASES = [c for c in R.LD_CASES if c[1] in LD_DIMS and c[2] == 0]
VEC_N, VEC_T = [1, 255, 256, 257, 2049], [1, 17, 64]


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def sentinels(size):
    return np.full(size, NAN64, F64)


def untouched(a):
    return bool((bits(a) == bits(np.array([NAN64]))[0]).all())


def twice(run):
    a, b = run(), run()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.dtype != F64 or same_bits(x, y), "two launches differ"
        assert x.dtype == F64 or np.array_equal(x, y), "two launches differ"
    return a


def kmm_inputs(D, rows, cols, T, square, integer, seed=0):
    """A, B with two sentinel rows behind them, V (T + 1 rows of ldv = cols + 3, sentinels behind column cols and in the
    last row), an integer diagonal."""
    rng = np.random.default_rng([91, D, rows, cols, T, int(square), seed])
    A = sentinels((rows + 2) * D)
    A[:rows * D] = rng.uniform(-1.0, 1.0, rows * D)
    B = None
    if not square:
        B = sentinels((cols + 2) * D)
        B[:cols * D] = rng.uniform(-1.0, 1.0, cols * D)
    ldv = cols + 3
    V = sentinels((T + 1) * ldv).reshape(T + 1, ldv)
    V[:T, :cols] = rng.integers(-8, 9, (T, cols)) if integer else rng.standard_normal((T, cols))
    diag = rng.integers(1, 6, rows).astype(F64) if square else None
    return A, B, V.reshape(-1), ldv, diag


@pytest.mark.parametrize("rows,cols,T,square", EXACT_SHAPES, ids=["%dx%d-T%d%s" % (s[0], s[1], s[2], "-sq" if s[3] else "")
                                                                  for s in EXACT_SHAPES])
@pytest.mark.parametrize("nslab", [1, 3, 8])
def test_kmm_exact(gpm, rows, cols, T, square, nslab):
    D = 3
    kp = R.exact_kp("generic", D)
    csum = sum(t["c"] for t in kp.terms)
    A, B, V, ldv, diag = kmm_inputs(D, rows, cols, T, square, True)
    rpad, ldo = -(-rows // 64) * 64, rows + 5
    Vm = V.reshape(T + 1, ldv)[:T, :cols]
    for max_blocks in (0, 2):  # 2: every workgroup walks several (row tile, slab) items wherever there are more than two
        part0, out0 = sentinels(nslab * T * rpad + 7), sentinels(T * ldo + 7)
        part, out = twice(lambda: gpm.kmm_check(kp.hook(gpm), A, rows, B, cols, V, ldv, T, diag, nslab, part0, out0, ldo,
                                                max_blocks=max_blocks))
        want = csum * Vm.sum(axis=1)[:, None] * np.ones((T, rows))
        if square:
            want = want + Vm * diag[None, :]
        body = out[:T * ldo].reshape(T, ldo)
        assert same_bits(body[:, :rows], want), "output"
        assert same_bits(body[:, rows:], np.zeros((T, ldo - rows))), "the padded rows of the output are zero"
        assert untouched(out[T * ldo:]) and untouched(part[nslab * T * rpad:])
        pm = part[:nslab * T * rpad].reshape(nslab, T, rpad)
        for s, (a, b) in enumerate(C.slab_columns(cols, nslab)):
            ws = csum * Vm[:, a:b].sum(axis=1)[:, None] * np.ones((T, rows))
            if square:
                ws[:, a:b] += Vm[:, a:b] * diag[None, a:b]
            assert same_bits(pm[s][:, :rows], ws), "partials of slab %d" % s
            assert same_bits(pm[s][:, rows:], np.zeros((T, rpad - rows))), "padded rows of slab %d" % s


def test_kmm_slab_rule(gpm):
    for rows, cols in [(1, 1), (64, 64), (600, 600), (4097, 4097), (16384, 16384), (64, 1048576), (1048576, 1048576)]:
        assert gpm.kmm_slabs(rows, cols) == C.kmm_slabs(rows, cols)


@pytest.mark.parametrize("case", LD_CASES, ids=[R.case_id(c) for c in LD_CASES])
def test_kmm_long_double(gpm, case):
    kp, D, n = R.kp_of(case), case[1], 193
    for T in (1, 17, 64):
        square = T == 17
        rows, cols = (n, n) if square else (n, 130)
        A, B, V, ldv, diag = kmm_inputs(D, rows, cols, T, square, False, seed=1)
        nslab, rpad, ldo = 3, -(-rows // 64) * 64, rows + 1
        part0, out0 = sentinels(nslab * T * rpad), sentinels(T * ldo)
        _, out = twice(lambda: gpm.kmm_check(kp.hook(gpm), A, rows, B, cols, V, ldv, T, diag, nslab, part0, out0, ldo))
        a = A[:rows * D].reshape(rows, D)
        b = a if square else B[:cols * D].reshape(cols, D)
        want, bound = C.kmm(kp, a, b, V.reshape(T + 1, ldv)[:T, :cols], diag)
        got = out.reshape(T, ldo)
        assert np.isfinite(got).all()
        assert same_bits(got[:, rows:], np.zeros((T, ldo - rows)))
        assert bound.max() <= 1e-10 * float(np.abs(want).max()), "the bound is too loose to judge by"
        err = np.abs(got[:, :rows].astype(LD) - want).astype(F64)
        ratio = float((err / bound).max())
        RATIOS[case[0]] = max(RATIOS.get(case[0], 0.0), ratio)
        assert (err <= bound).all(), "%s T %d: worst |err| / bound = %g" % (R.case_id(case), T, ratio)


def test_print_the_worst_ratios():
    for fam in sorted(RATIOS):
        print("kmm %-12s worst |err| / bound = %.3g" % (fam, RATIOS[fam]))


# ---- the column-wise kernels ---------------------------------------------------------------------------------------------------
def block(rng, T, ld, n, lo=-9, hi=10):
    """T rows of ld with integers on the first n columns, sentinels behind them and behind the block."""
    a = sentinels(T * ld + 3)
    m = a[:T * ld].reshape(T, ld)
    m[:, :n] = rng.integers(lo, hi, (T, n))
    return a


def state(T, frozen=None):
    sc, st = np.zeros(6 * 64), np.zeros(4 * 64, dtype=np.int32)
    if frozen is not None:
        st[:T] = frozen
    return sc, st


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("T", VEC_T)
def test_dots_and_decisions(gpm, n, T):
    rng = np.random.default_rng([92, n, T])
    ld = n + 2
    A, B = block(rng, T, ld, n), block(rng, T, ld, n)
    Am, Bm = A[:T * ld].reshape(T, ld)[:, :n], B[:T * ld].reshape(T, ld)[:, :n]
    dots = (Am * Bm).sum(axis=1)
    nb = gpm.cg_dot_blocks(n)
    assert nb == max(1, min(-(-n // 2048), 512))
    part0 = sentinels(T * nb + 5)
    sc0, st0 = state(T)
    sc0[:] = NAN64
    part, out, sc, st = twice(lambda: gpm.cg_dots_check(A, B, ld, n, T, "plain", 0, 1.0, part0, sentinels(T + 2), sc0, st0))
    assert same_bits(out[:T], dots) and untouched(out[T:]) and untouched(part[T * nb:])
    assert same_bits(part[:T * nb].reshape(T, nb).sum(axis=1), dots)
    assert untouched(sc) and np.array_equal(st, st0), "plain mode leaves the state alone"
    # |b|^2: a zero column is frozen from the start
    Z = A.copy()
    Z[:T * ld].reshape(T, ld)[T // 2, :n] = 0.0
    _, _, sc, st = gpm.cg_dots_check(Z, Z, ld, n, T, "bnorm", 0, 1.0, part0, None, *state(T))
    zz = (Z[:T * ld].reshape(T, ld)[:, :n] ** 2).sum(axis=1)
    assert same_bits(sc[3 * 64:3 * 64 + T], zz) and same_bits(sc[4 * 64:4 * 64 + T], zz)
    assert np.array_equal(st[:T], (zz == 0).astype(np.int32)) and not st[64:].any()
    # p^T q: a = rho / dot on live columns, 0 on frozen ones; a non-positive dot marks the column bad and freezes it
    frozen = (np.arange(T) % 3 == 1).astype(np.int32)
    sc1, st1 = state(T, frozen)
    sc1[:T] = 8.0 * (1 + np.arange(T))
    _, _, sc, st = gpm.cg_dots_check(A, B, ld, n, T, "pq", 4, 1.0, part0, None, sc1, st1)
    ok = (dots > 0) & (frozen == 0)
    assert same_bits(sc[64:64 + T], np.where(ok, sc1[:T] / np.where(ok, dots, 1.0), 0.0))
    assert same_bits(sc[5 * 64:5 * 64 + T], dots)
    assert np.array_equal(st[2 * 64:2 * 64 + T], ((dots <= 0) & (frozen == 0)).astype(np.int32))
    assert np.array_equal(st[:T], np.maximum(frozen, (dots <= 0).astype(np.int32)))
    # |r|^2 and the freeze test: live columns record the iteration; sqrt(dot) <= tol sqrt(|b|^2) freezes
    sc2, st2 = state(T, frozen)
    aa = (Am * Am).sum(axis=1)
    sc2[3 * 64:3 * 64 + T] = np.where(np.arange(T) % 2 == 0, 4.0 * aa, aa / 4.0)  # tol = 1/2: even columns freeze exactly at the bound
    sc2[4 * 64:4 * 64 + T] = -1.0
    _, _, sc, st = gpm.cg_dots_check(A, A, ld, n, T, "rr", 7, 0.5, part0, None, sc2, st2)
    live = frozen == 0
    assert same_bits(sc[4 * 64:4 * 64 + T], np.where(live, aa, -1.0))
    assert np.array_equal(st[64:64 + T], np.where(live, 7, 0).astype(np.int32))
    assert np.array_equal(st[:T], np.where(live, (np.arange(T) % 2 == 0) | (aa == 0), 1).astype(np.int32))
    # beta = dot / rho and rho = dot on live columns; beta = 0 on frozen ones, whose rho stays
    sc3, st3 = state(T, frozen)
    sc3[:T] = 4.0
    sc3[2 * 64:2 * 64 + T] = 99.0
    _, _, sc, st = gpm.cg_dots_check(A, B, ld, n, T, "beta", 7, 0.5, part0, None, sc3, st3)
    assert same_bits(sc[2 * 64:2 * 64 + T], np.where(live, dots / 4.0, 0.0))
    assert same_bits(sc[:T], np.where(live, dots, 4.0)) and np.array_equal(st, st3)
    # rho0
    _, _, sc, st = gpm.cg_dots_check(A, B, ld, n, T, "rho0", 0, 0.5, part0, None, *state(T))
    assert same_bits(sc[:T], dots)


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("T", VEC_T)
def test_vector_updates(gpm, n, T):
    rng = np.random.default_rng([93, n, T])
    ld = n + 1
    x, r, p, q, z = (block(rng, T, ld, n) for _ in range(5))
    frozen = (np.arange(T) % 4 == 2).astype(np.int32)
    sc, st = state(T, frozen)
    sc[64:64 + T] = rng.integers(-4, 5, T) / 4.0      # a
    sc[2 * 64:2 * 64 + T] = rng.integers(-4, 5, T) / 2.0  # beta
    sc[64 + T:2 * 64] = NAN64
    live = (frozen == 0)[:, None]

    def m(a):
        return a[:T * ld].reshape(T, ld)[:, :n]

    x1, r1 = twice(lambda: gpm.cg_update_xr_check(x, r, p, q, ld, n, T, sc, st))
    a = sc[64:64 + T][:, None]
    assert same_bits(m(x1), np.where(live, m(x) + a * m(p), m(x))) and same_bits(m(r1), np.where(live, m(r) - a * m(q), m(r)))
    p1 = twice(lambda: gpm.cg_update_p_check(p, z, ld, n, T, sc, st))
    assert same_bits(m(p1), np.where(live, m(z) + sc[2 * 64:2 * 64 + T][:, None] * m(p), m(p)))
    w = rng.integers(1, 5, n).astype(F64)
    wpad = np.concatenate([w, sentinels(2)])
    o1 = twice(lambda: gpm.cg_scale_check(x, wpad, q, ld, n, T, sentinels(T * ld + 3)))
    assert same_bits(m(o1), m(x) * w[None, :] - m(q))
    o2 = gpm.cg_scale_check(x, None, q, ld, n, T, sentinels(T * ld + 3))
    o3 = gpm.cg_scale_check(x, wpad, None, ld, n, T, sentinels(T * ld + 3))
    assert same_bits(m(o2), m(x) - m(q)) and same_bits(m(o3), m(x) * w[None, :])
    for got in (x1, r1, p1, o1, o2, o3):  # nothing beyond the n columns of the T rows is written
        assert untouched(got[:T * ld].reshape(T, ld)[:, n:]) and untouched(got[T * ld:])
    s1 = gpm.cg_status_check(T, st)
    assert s1[3 * 64] == int((frozen == 0).sum()) and s1[3 * 64 + 1] == 0
    st[2 * 64 + T - 1] = 1
    assert gpm.cg_status_check(T, st)[3 * 64 + 1] == T


@pytest.mark.parametrize("n,r,T", [(1, 0, 1), (257, 0, 17), (63, 5, 1), (300, 16, 17), (2049, 33, 64), (5000, 40, 3)])
def test_preconditioner(gpm, n, r, T):
    """Z = P^-1 R on a given scaled factor against the reference's Woodbury form, and C = I + Ls^T Ls; a column's bits do
    not depend on the columns beside it."""
    rng = np.random.default_rng([94, n, r, T])
    ldn, ld, rp = n + 3, n + 2, -(-r // 16) * 16
    d = rng.uniform(0.5, 2.0, n)
    dis = np.concatenate([1.0 / np.sqrt(d), sentinels(1)])
    L = rng.standard_normal((n, r)) / np.sqrt(max(r, 1))
    Rb = sentinels(T * ld + 1)
    Rb[:T * ld].reshape(T, ld)[:, :n] = rng.standard_normal((T, n))
    Rm = Rb[:T * ld].reshape(T, ld)[:, :n]
    Ls = Cinv = None
    if r:
        Ls = sentinels(r * ldn)
        Ls.reshape(r, ldn)[:, :n] = (L * dis[:n, None]).T
        Cm = np.eye(rp)
        Cm[:r, :r] += (L * dis[:n, None]).T @ (L * dis[:n, None])
        Cinv = np.ascontiguousarray(np.linalg.inv(Cm)).reshape(-1)
    z0 = sentinels(T * ld + 1)
    if r:
        Z, Cg = twice(lambda: gpm.cg_precond_check(Ls, ldn, n, r, dis, Cinv, Rb, ld, T, z0, C=sentinels(rp * rp)))
        scale = np.abs(Cm).max()
        assert np.abs(Cg.reshape(rp, rp) - Cm).max() <= 4 * C.gamma(n) * r * scale
        assert same_bits(Cg.reshape(rp, rp), Cg.reshape(rp, rp).T.copy())
    else:
        Z = twice(lambda: gpm.cg_precond_check(None, ldn, n, 0, dis, None, Rb, ld, T, z0))
    Ls_m = L * dis[:n, None]
    Rp = Rm * dis[:n]
    Ci = np.linalg.inv(Cm)[:r, :r] if r else None  # (the padding of C is the identity)
    want = dis[:n] * (Rp - (Ci @ (Rp @ Ls_m).T).T @ Ls_m.T) if r else Rp * dis[:n]
    got = Z[:T * ld].reshape(T, ld)
    # every sum has at most n + r terms of magnitude sum |.|: a few gamma_{n + r} of the magnitudes, taken generously
    mag = np.abs(Rp) + (np.abs(Ci) @ (np.abs(Rp) @ np.abs(Ls_m)).T).T @ np.abs(Ls_m).T if r else np.abs(Rp)
    assert (np.abs(got[:, :n] - want) <= 8 * C.gamma(n + r + 4) * (mag * dis[:n]).max()).all()
    assert untouched(got[:, n:]) and untouched(Z[T * ld:])
    if T > 1:  # the first column alone: the same bits
        one = gpm.cg_precond_check(Ls, ldn, n, r, dis, Cinv, Rb[:ld].copy(), ld, 1, sentinels(ld))
        assert same_bits(one[:n], got[0, :n])
