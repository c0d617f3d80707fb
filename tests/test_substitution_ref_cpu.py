"""The host references of tests/substitution_ref.py against independent computations (no GPU): what the GPU tests of the
substitution kernels (tests/test_substitution_kernels.py) are judged by must itself be right."""
import numpy as np
import pytest

import substitution_ref as R

P = R.P


def true_inverse_operands(npad, m, seed):
    """A well-conditioned lower-triangular T whose diagonal blocks' TRUE inverses serve as Dinv."""
    rng = np.random.default_rng(seed)
    T = np.tril(rng.uniform(-1, 1, (npad, npad))) / np.sqrt(npad)
    T[np.diag_indices(npad)] = 1.0 + rng.uniform(0, 1, npad)
    nb = npad // P
    Dinv = np.stack([np.linalg.inv(T[B * P:(B + 1) * P, B * P:(B + 1) * P]) for B in range(nb)])
    return T, Dinv, rng.standard_normal((npad, m))


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_true_inverses_give_the_triangular_solve(backward):
    T, Dinv, b = true_inverse_operands(768, 3, 5)
    V, _, E, _ = R.substitute(T, Dinv, b, "ld", backward=backward)
    want = np.linalg.solve(T.T if backward else T, b)
    # both sides carry the conditioning of T (about 10): 1e-12 is four digits above either's rounding
    assert np.abs(V.astype(np.float64) - want).max() <= 1e-12 * np.abs(want).max()
    assert E.max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_integer_mode_equals_long_double_mode_on_integer_data(backward):
    L, Dinv, b = R.exact_operands(768, 5, 11)
    Vi, Wi = R.substitute(L, Dinv, b, "int", backward=backward)
    Vl, Wl, E, _ = R.substitute(L, Dinv, b, "ld", backward=backward)
    assert np.abs(Vi).max() < 2 ** 24  # below 2^64: long doubles hold every partial sum exactly too
    assert np.array_equal(Vi.astype(np.longdouble), Vl) and np.array_equal(Wi.astype(np.longdouble), Wl)
    Vo, Wo = R.substitute(L[:512, :512], Dinv[:2], b[:512, :2], "object", backward=backward)
    Vs, Ws = R.substitute(L[:512, :512], Dinv[:2], b[:512, :2], "int", backward=backward)
    assert all(int(x) == int(y) for x, y in zip(Vo.ravel(), Vs.ravel()))
    assert all(int(x) == int(y) for x, y in zip(Wo.ravel(), Ws.ravel()))


@pytest.mark.parametrize("npad,log2max", [(768, 30), (1280, 46)])
def test_integer_operands_keep_their_headroom(npad, log2max):
    """Every partial sum below 2^30 at npad = 768 and 2^46 at 1280, over absolute values even (the solutions themselves
    reach 2^22 and 2^36): far from 2^53.  The substitute() call asserts the 2^53 headroom itself; this pins how much
    is left, so that a change of the operands that eats it shows here first."""
    L, Dinv, b = R.exact_operands(npad, 64, 100 + npad)
    V, W = R.substitute(L, Dinv, b, "int")
    nb = npad // P
    Va = np.abs(V).astype(np.float64)
    worst = 0.0
    for B in range(nb):
        mag = np.abs(b[B * P:(B + 1) * P]) + np.abs(L[B * P:(B + 1) * P, :B * P]) @ Va[:B * P]
        worst = max(worst, (np.abs(Dinv[B]) @ mag).max())
    assert worst < 2.0 ** log2max, np.log2(worst)


def test_integer_mode_refuses_lost_headroom():
    L, Dinv, b = R.exact_operands(512, 2, 3)
    with pytest.raises(AssertionError, match="headroom"):
        R.substitute(L, Dinv, b * 2.0 ** 45, "int")
    with pytest.raises(AssertionError, match="integer"):
        R.substitute(L, Dinv, b + 0.5, "int")


def test_single_steps_compose_to_the_chain():
    L, Dinv, b = R.exact_operands(768, 1, 21)
    V, _ = R.substitute(L, Dinv, b, "int")
    w = b[:, 0].copy()
    z = np.zeros(768, np.int64)
    for bk in range(3):
        zb, wn = R.fwd_step(L, Dinv, bk, w, "int")
        z[bk * P:(bk + 1) * P], w = zb, wn.astype(np.float64)
    assert np.array_equal(z, V[:, 0])
    A, _ = R.substitute(L, Dinv, b, "int", backward=True)
    w = b[:, 0].copy()
    a = np.zeros(768, np.int64)
    for bk in (2, 1, 0):
        ab, wn = R.bwd_step(L, Dinv, bk, w, "int")
        a[bk * P:(bk + 1) * P], w = ab, wn.astype(np.float64)
    assert np.array_equal(a, A[:, 0])


def test_layouts_round_trip():
    rng = np.random.default_rng(7)
    V = rng.standard_normal((512, 32))
    for width, m in ((16, 9), (16, 16), (32, 17), (32, 32)):
        raw = R.encode_paired(V[:, :m], width)
        got = R.decode_paired(raw, 512, width)
        assert np.array_equal(got[:, :m], V[:, :m]) and not got[:, m:].any()
        # the documented address: element (k, j) at ((k >> 1) * width + j) * 2 + (k & 1)
        flat = np.frombuffer(raw, np.float64)
        for k, j in ((0, 0), (1, 0), (2, 3), (511, m - 1), (300, 1)):
            assert flat[((k >> 1) * width + j) * 2 + (k & 1)] == V[k, j]
    for width, m in ((1, 1), (2, 2), (4, 3), (8, 5), (8, 8)):
        raw = R.encode_compact(V[:, :m], width)
        assert np.array_equal(R.decode_compact(raw, 512, width)[:, :m], V[:, :m])
        assert np.frombuffer(raw, np.float64)[77 * width + m - 1] == V[77, m - 1]
    raw = R.encode_granule(V[:, 0])
    got, tags = R.decode_granule(raw, 512)
    assert np.array_equal(got[:, 0], V[:, 0]) and (tags == 1).all()
    words = np.frombuffer(raw, np.uint32).reshape(512, 4)
    bits = V[:, 0].view(np.uint64)
    assert np.array_equal(words[:, 1], (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32))  # low word second
    assert np.array_equal(words[:, 3], (bits >> np.uint64(32)).astype(np.uint32))  # high word last
    assert np.array_equal(R.decode_solution(raw, R.TS_SOL_GRANULE, 1, 0, 512), V[:, :1])
    with pytest.raises(AssertionError, match="tag"):
        R.decode_solution(R.encode_granule(V[:, 0], tag=2), R.TS_SOL_GRANULE, 1, 0, 512)
    pad = np.concatenate([np.zeros(48, np.uint8), R.encode_compact(V[:, :4], 4)])
    assert np.array_equal(R.decode_solution(pad, R.TS_SOL_COMPACT, 4, 48, 512), V[:, :4])


def test_a_dropped_low_word_is_far_outside_the_bound():
    """What the full-mantissa cases are for: a granule that loses its low word is off by up to 2^-20 relative."""
    L, Dinv, b = R.mantissa_operands(512, 1, 9)
    V, _, E, _ = R.substitute(L, Dinv, b, "ld")
    v = V.astype(np.float64)[:, 0]
    raw = R.encode_granule(v).copy()
    np.frombuffer(raw, np.uint32).reshape(-1, 4)[:, 1] = 0
    got, _ = R.decode_granule(raw, 512)
    assert (np.abs(got[:, 0] - v) > 1e3 * E[:, 0]).sum() > 500


def test_expected_solution_table():
    want = {(64, 0, 1): ("granule", 2, 1), (64, 32, 1): ("NT1-MC1", 1, 1), (64, 0, 2): ("NT1-MC2", 1, 2),
            (64, 0, 3): ("NT1-MC4", 1, 4), (64, 0, 4): ("NT1-MC4", 1, 4), (64, 0, 5): ("NT1-MC8", 1, 8),
            (64, 0, 8): ("NT1-MC8", 1, 8), (64, 0, 9): ("NT1-MC16", 0, 16), (64, 0, 16): ("NT1-MC16", 0, 16),
            (64, 0, 17): ("NT2-MC32", 0, 32), (64, 32, 32): ("NT2-MC32", 0, 32), (32, 0, 1): ("NT1-MC1", 1, 1),
            (32, 0, 7): ("NT1-MC8", 1, 8)}
    for (prec, j0, cnt), exp in want.items():
        assert R.expected_solution(prec, j0, cnt) == exp


@pytest.mark.parametrize("npad,m,seed,as_float", R.MANTISSA_CASES,
                         ids=["n%d-m%d-s%d-%s" % (c[0], c[1], c[2], "f32" if c[3] else "f64") for c in R.MANTISSA_CASES])
def test_running_bound_holds_and_stays_small(npad, m, seed, as_float):
    """For every random case of the GPU file: a plain fp64 numpy run of the same recurrence lies inside the running
    bound, and the bound is small -- max(e) <= 1e-10 max |V| -- so that it cannot hide a failure."""
    L, Dinv, b = R.mantissa_operands(npad, m, seed, as_float=as_float)
    V, W, E, _ = R.substitute(L, Dinv, b, "ld")
    assert E.max() <= 1e-10 * float(np.abs(V).max()), E.max() / float(np.abs(V).max())
    if npad <= 1280:
        V64, _ = R.substitute(L, Dinv, b, "f64")
        err = np.abs(V64.astype(np.longdouble) - V).astype(np.float64)
        assert (err <= E).all(), (err / E).max()
        assert err.max() > 0  # the comparison is not vacuous: fp64 does round here
        Vb, _, Eb, _ = R.substitute(L, Dinv, b[:, :1], "ld", backward=True)
        Vb64, _ = R.substitute(L, Dinv, b[:, :1], "f64", backward=True)
        assert (np.abs(Vb64.astype(np.longdouble) - Vb).astype(np.float64) <= Eb).all()
        assert Eb.max() <= 1e-10 * float(np.abs(Vb).max())


def test_hooks_refuse_before_the_device():
    """A test's mistake comes back as GOGP_EARG (1) before the device is touched -- so this runs without one."""
    from gogp_amd import gp
    L = np.zeros(256 * 264)
    D = np.zeros(256 * 256)
    v = np.zeros(256)
    for kw, dtp, direction in ((dict(k=2, bstride=256 * 264), np.float32, "fwd"), (dict(k=2, bstride=256 * 264), np.float64, "bwd")):
        Lk = np.zeros(2 * 256 * 264, dtp)
        Dk = np.zeros(256 * 264 + 256 * 256, dtp)
        with pytest.raises(gp.GogpError) as ei:
            gp.trsv_steps_check(direction, 256, Lk, 264, Dk, 0, 0, np.zeros(256 * 264 + 256), np.zeros(256 * 264 + 256), **kw)
        assert ei.value.code == 1
    with pytest.raises(gp.GogpError) as ei:  # KsT does not cover the 16 rows the instance reads
        gp.trsm_small_check(256, L, 264, D, np.zeros(2 * 264), 264, 0, 2, np.zeros(2))
    assert ei.value.code == 1
    with pytest.raises(gp.GogpError) as ei:  # step outside the chain
        gp.trsv_steps_check("fwd", 256, L, 264, D, 0, 1, v, v)
    assert ei.value.code == 1
    arena = np.zeros(3 * 65536)
    for prods in ([(0, 256, 65536, 256, 131072, 256, 48)], [(0, 256, 65536, 256, 131072 + 8, 256, 32)],
                  [(0, 256, 65536, 256, 131072, 256, 32)] * 7):
        with pytest.raises(gp.GogpError) as ei:  # K not a multiple of 32; C outside the arena; seven products
            gp.blockmm_check(arena, prods)
        assert ei.value.code == 1
