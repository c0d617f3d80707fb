"""The kernels of csrc/hessian.hip alone, through the hooks gogp_test_hess_* and their product launchers (run with -m gpu),
over the descriptor space of tests/hessian_ref.py: ALL_CASES.

Inputs: X, and K^-1 and alpha of the long-double factorisation rounded to float64 -- the numbers the device is given, which
the long-double references take as exact.  K^-1 goes up as its n rows of ld = n + 3 with NaN above the diagonal and behind
column n; every output starts as NaN; a matrix M that is an input is NaN outside its leading n x n.

Bounds.  The tile product keeps tests/test_hessian_kernel.py's: |M - ref|_F <= n eps |K^-1|_F |K_s|_F.  Pure sums of
products of given numbers (matvec, dots, traces, quad): gamma(k) x the sum of the terms' magnitudes, k the length of the sum
(tests/grad_reduce_ref.py: gamma).  What evaluates the similarity (pair, kvec): the scheme of
tests/test_vecchia_blocks_gpu.py.  A quantity -- one moment's tile sums, one slot's vector b -- is held element by element to
FACTOR = 8 x the float64 restatement's own largest difference from the long-double values (its share of the quantity's
largest magnitude, times that magnitude); the restatement carries the summation's error, so nothing is added for it.
The pair kernel's tile sums alone have a floor under that, as the end-to-end test has: gamma(k) x the sum of the magnitudes
of the k pairs' terms in the tile.  Without it 17 of the 772 non-vanishing moments missed on an MI355X, by up to 14.2 x, all
in launches of one or three tiles (n <= 65): a tile sums up to 4096 terms whose weight
alpha_i alpha_j - K^-1_ij changes sign, 1 / 100 .. 1 / 1000 of their magnitudes is left, and with so few tiles the
restatement's difference is one sample of such a sum's rounding, which can lie far below the typical one.  The floor then
governs most tiles (ratios of 0.001 .. 0.1); both ratios are printed.  A
moment's total, the launch's sum over its nb tiles, is held to (FACTOR x share x nb + gamma(nb + 1)) x the sum of the tiles'
magnitudes -- for the same reason the sums of their summands' magnitudes: with the tiles' own |sum| the one-tile launches
above missed in 12 of 772 totals, by up to 7.6 x (the total is the tile).  The restatement's difference must itself lie in (0, 1e-10); a quantity that vanishes identically must vanish
on the device.  Every figure is printed before it is asserted (-s); the worst ratios recorded on an MI355X: DESIGN.md
section 4, the Hessian's entry."""
import functools

import numpy as np
import pytest

import grad_reduce_ref as G
import hessian_ref as R
from gogp_amd import gp as gpm
from gogp_amd import hessian

pytestmark = pytest.mark.gpu
LD, F64 = np.longdouble, np.float64
NAN = np.nan
FACTOR = 8.0
NS = [1, 63, 64, 65, 129, 200]
#: the sizes every case runs at (one row past two tiles) and the cases that walk all of NS: an odd and an even D, a
#: periodic term with ARD lengths, the repeated rows
N_ALL = 129
SWEEP = ["matern52-u-D1", "ard-periodic", "ard-m52-D4", "duplicates"]


def npad_of(n, spare=False):
    return -(-n // 64) * 64 + (64 if spare else 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def stored(Kinv, n, ld):
    """n rows of ld: the lower triangle, NaN above the diagonal and behind column n."""
    out = np.full((n, ld), NAN)
    out[:, :n] = np.where(np.tril(np.ones((n, n), bool)), Kinv, NAN)
    return out


@functools.lru_cache(maxsize=None)
def problem(name, n):
    p = R.kernel_inputs(name, n)
    return dict(p, hook=p["kp"].hook(gpm), ld=n + 3, stored=stored(p["Kinv"], n, n + 3))


def groups_of(p):
    """(term, [(type, dim)], first slot) per group."""
    return [(t, [s[1:3] for s in p["slots"][f:f + k]], f) for t, f, k in p["groups"]]


def tyd(g):
    return [a for a, _ in g], [b for _, b in g]


def share_of(what, want, w64):
    """(share, mag) of one quantity: the restatement's largest difference from the long-double values over the quantity's
    largest magnitude; (0, 0) for a quantity that vanishes identically."""
    want = np.asarray(want)
    mag = float(np.abs(want).max())
    if mag == 0:
        assert not np.asarray(w64).any(), what
        return 0.0, 0.0
    share = float(np.abs(np.asarray(w64, F64).astype(LD) - want).max()) / mag
    assert 0 < share < 1e-10, "%s: the restatement's own difference %.3g" % (what, share)
    return share, mag


def judge(what, got, want, w64, floor=None):
    """One quantity element by element: |got - want| <= FACTOR x share x mag, or, where a floor is given (the pair kernel's
    tile sums), that element's floor if it is larger.  A quantity that vanishes identically must vanish on the device.
    Prints the ratio, and beside it the ratio without the floor.  Returns the ratio."""
    got = np.asarray(got, F64)
    assert np.isfinite(got).all(), what
    share, mag = share_of(what, want, w64)
    if mag == 0:
        assert not got.any(), what
        return 0.0
    err = np.abs(got.astype(LD) - np.asarray(want)).astype(F64)
    strict = float(err.max()) / (FACTOR * share * mag)
    ratio = strict if floor is None else float((err / np.maximum(FACTOR * share * mag, floor)).max())
    print("%s: |err| %.3g, allowed %.3g, ratio %.3f%s" % (what, err.max(), FACTOR * share * mag, ratio,
                                                         "" if floor is None else " (%.3f without the floor)" % strict))
    assert ratio <= 1.0, what
    return ratio


def judge_sum(what, got, want_blocks, w64_blocks, summands):
    """A launch-wide sum over nb blocks, which the launch returns whole: |got - sum| <= (FACTOR x share x nb + gamma(nb + 1))
    x the sum of the blocks' magnitudes, the share taken over the blocks' contributions.  A block's magnitude is the sum of
    its summands' magnitudes (`summands`, one per block); the ratio with |block| in its place is printed beside it."""
    want_blocks = np.asarray(want_blocks)
    nb = len(want_blocks)
    share, mag = share_of(what, want_blocks, w64_blocks)
    if mag == 0:
        assert got == 0, what
        return 0.0
    err = abs(float(LD(got) - want_blocks.sum()))
    rel = FACTOR * share * nb + G.gamma(nb + 1)
    allowed = rel * float(np.sum(summands))
    print("%s: |err| %.3g, allowed %.3g, ratio %.3f (%.3f with the blocks' own magnitudes)" %
          (what, err, allowed, err / allowed, err / (rel * float(np.abs(want_blocks).sum()))))
    assert np.isfinite(got) and err <= allowed, what
    return err / allowed


def sum_bound(what, got, want, k, terms_mag):
    """A pure sum of k products: |got - want| <= gamma(k) x the sum of the terms' magnitudes."""
    got, want, terms_mag = np.asarray(got, F64), np.asarray(want), np.asarray(terms_mag, F64)
    err = np.abs(got.astype(LD) - want).astype(F64)
    allowed = G.gamma(k) * terms_mag
    assert np.isfinite(got).all(), what
    zero = allowed == 0
    assert not err[zero].any(), what
    ratio = float((err[~zero] / allowed[~zero]).max()) if (~zero).any() else 0.0
    print("%s: |err| %.3g, ratio %.3f" % (what, err.max(), ratio))
    assert ratio <= 1.0, what
    return ratio


# ---- hess_kmm_kernel ---------------------------------------------------------------------------------------------------------
def run_kmm(name, n, npad, twice=False):
    p = problem(name, n)
    Ks = R.slot_matrices(p)
    Kl = p["Kinv"].astype(LD)
    worst = 0.0
    for t, g, first in groups_of(p):
        ty, dm = tyd(g)
        M0 = np.full((len(g) + 1, npad, npad), NAN)  # one matrix more than the group has slots
        M = hessian.kmm_check(p["hook"], t, ty, dm, p["X"], n, npad, p["stored"], p["ld"], M0, device=0).reshape(M0.shape)
        if twice:
            again = hessian.kmm_check(p["hook"], t, ty, dm, p["X"], n, npad, p["stored"], p["ld"], M0, device=0)
            assert np.array_equal(bits(M), bits(again.reshape(M0.shape)))
        assert np.isnan(M[len(g)]).all(), "a slot behind grp.n was written"
        for q in range(len(g)):
            ref = Kl @ Ks[first + q]
            err = float(np.linalg.norm((M[q, :n, :n] - ref).astype(F64)))
            bound = n * 2.0 ** -52 * np.linalg.norm(p["Kinv"]) * float(np.linalg.norm(Ks[first + q].astype(F64)))
            print("kmm %s n %d term %d slot %d (type %d dim %d): |M - ref|_F %.3e, bound %.3e" %
                  (name, n, t, first + q, ty[q], dm[q], err, bound))
            assert err <= bound
            worst = max(worst, err / bound) if bound else worst
            pad = M[q].copy()
            pad[:n, :n] = 0.0
            assert not pad.any(), "whole tiles are written: exact zeros from row / column n on"
    print("kmm %s n %d: worst ratio %.3f" % (name, n, worst))


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_kmm_every_group_of_every_case(name):
    run_kmm(name, N_ALL, npad_of(N_ALL), twice=name == "four")


@pytest.mark.parametrize("n", NS)
def test_kmm_sizes(n):
    for name in SWEEP:
        run_kmm(name, n, npad_of(n, spare=n == 65))


# ---- hess_pair_kernel, hess_sum_kernel ------------------------------------------------------------------------------------------
def run_pair(name, n, npad, twice=False):
    p = problem(name, n)
    gs = groups_of(p)
    nt = npad // 64
    ntl = nt * (nt + 1) // 2
    pairs = R.tile_sums(np.tril(np.ones((n, n))), n, npad=npad)  # the pairs j <= i < n a tile sums
    worst = 0.0
    for ia, (ta, ga, _) in enumerate(gs):
        for tb, gb, _ in gs[ia:]:
            if ta != tb:
                continue
            args = (p["hook"], ta, *tyd(ga), *tyd(gb), p["X"], p["alpha"], n, npad, p["stored"], p["ld"],
                    np.full(ntl * R.HESS_NMOM, NAN), np.full(R.HESS_NMOM, NAN))
            part, out = hessian.pair_check(*args, device=0)
            if twice:
                part2, out2 = hessian.pair_check(*args, device=0)
                assert np.array_equal(bits(part), bits(part2)) and np.array_equal(bits(out), bits(out2))
            part = part.reshape(ntl, R.HESS_NMOM)
            assert np.isfinite(part).all() and np.isfinite(out).all()
            want, mag = R.moments(p, ta, ga, gb, "ld", npad)
            w64, _ = R.moments(p, ta, ga, gb, "f64", npad)
            what = "pair %s n %d term %d groups %s x %s" % (name, n, ta, ga, gb)
            # every moment is a quantity of its own: its tiles element by element, its total as the launch's sum over them
            for m in range(R.HESS_NMOM):
                worst = max(worst, judge("%s moment %d tiles" % (what, m), part[:, m], want[:, m], w64[:, m],
                                         G.gamma(pairs) * mag[:, m]))
                worst = max(worst, judge_sum("%s moment %d sum" % (what, m), out[m], want[:, m], w64[:, m], mag[:, m]))
            # moments behind ga.n / gb.n are exactly 0
            G_ = R.HESS_G
            dead = [1 + q for q in range(len(ga), G_)] + [1 + 2 * G_ + q for q in range(len(ga), G_)]
            dead += [1 + 3 * G_ + q for q in range(len(ga), G_)] + [1 + G_ + q for q in range(len(gb), G_)]
            dead += [1 + 4 * G_ + q for q in range(len(gb), G_)]
            dead += [1 + 5 * G_ + a * G_ + b for a in range(G_) for b in range(G_) if a >= len(ga) or b >= len(gb)]
            assert not part[:, dead].any() and not out[dead].any(), what
    print("pair %s n %d: worst ratio %.3f" % (name, n, worst))


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_pair_every_group_pair_of_every_case(name):
    run_pair(name, N_ALL, npad_of(N_ALL), twice=name == "ard-periodic")


@pytest.mark.parametrize("n", NS)
def test_pair_sizes(n):
    for name in SWEEP:
        run_pair(name, n, npad_of(n, spare=n == 65))


# ---- hess_kvec_kernel ----------------------------------------------------------------------------------------------------------
def run_kvec(name, n, npad, twice=False):
    p = problem(name, n)
    Ks, K64 = R.slot_matrices(p), R.slot_matrices(p, "f64")
    a = p["alpha"]
    ldb = npad + 5
    worst = 0.0
    for t, g, first in groups_of(p):
        b0 = np.full((len(g) + 1, ldb), NAN)
        args = (p["hook"], t, *tyd(g), p["X"], a, n, npad, b0, ldb)
        b = hessian.kvec_check(*args, device=0).reshape(b0.shape)
        if twice:
            assert np.array_equal(bits(b), bits(hessian.kvec_check(*args, device=0).reshape(b0.shape)))
        assert np.isnan(b[len(g)]).all() and np.isnan(b[:, npad:]).all(), "written behind g.n or behind npad"
        assert not b[:len(g), n:npad].any(), "rows n .. npad are exact zeros"
        for q in range(len(g)):
            K = Ks[first + q]
            worst = max(worst, judge("kvec %s n %d slot %d" % (name, n, first + q), b[q, :n], K @ a.astype(LD),
                                     K64[first + q] @ a))
    print("kvec %s n %d: worst ratio %.3f" % (name, n, worst))


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_kvec_every_group_of_every_case(name):
    run_kvec(name, N_ALL, npad_of(N_ALL), twice=name == "four")


@pytest.mark.parametrize("n", NS)
def test_kvec_sizes(n):
    for name in SWEEP:
        run_kvec(name, n, npad_of(n, spare=n == 65))


def runs():
    """(name, n, npad) of every launch of the pair and kvec tests."""
    return [(name, N_ALL, npad_of(N_ALL)) for name in R.ALL_CASES] + [(name, n, npad_of(n, n == 65)) for n in NS for name in SWEEP]


def check_shares(name, n, npad):
    """Without a device (tests/test_hessian_ref_cpu.py): the restatement's share of every quantity the pair and kvec tests
    judge at this launch lies in (0, 1e-10), or the quantity vanishes identically."""
    p = problem(name, n)
    gs = groups_of(p)
    for ia, (ta, ga, _) in enumerate(gs):
        for tb, gb, _ in gs[ia:]:
            if ta == tb:
                want, w64 = R.moments(p, ta, ga, gb, "ld", npad)[0], R.moments(p, ta, ga, gb, "f64", npad)[0]
                for m in range(R.HESS_NMOM):
                    share_of("pair %s n %d %s x %s moment %d" % (name, n, ga, gb, m), want[:, m], w64[:, m])
    for q, (K, K64) in enumerate(zip(R.slot_matrices(p), R.slot_matrices(p, "f64"))):
        share_of("kvec %s n %d slot %d" % (name, n, q), K @ p["alpha"].astype(LD), K64 @ p["alpha"])


# ---- the pure sums: given numbers ---------------------------------------------------------------------------------------------
def given(n, npad, S, seed):
    """S matrices (NaN outside n x n), a symmetric K^-1 (stored: n rows of ld = n + 3), alpha."""
    rng = np.random.default_rng([2887, n, npad, S, seed])
    M = np.full((S, npad, npad), NAN)
    M[:, :n, :n] = rng.standard_normal((S, n, n))
    K = rng.standard_normal((n, n))
    K = K + K.T
    return M, K, stored(K, n, n + 3), rng.standard_normal(n)


@pytest.mark.parametrize("n", NS)
def test_matvec(n):
    for S, spare in ((1, False), (3, n == 65)):
        npad = npad_of(n, spare)
        M, _, _, a = given(n, npad, S, 1)
        c0 = np.full((S, npad), NAN)
        c = hessian.matvec_check(M, a, n, npad, S, c0, device=0).reshape(c0.shape)
        assert np.array_equal(bits(c), bits(hessian.matvec_check(M, a, n, npad, S, c0, device=0).reshape(c0.shape)))
        assert not c[:, n:].any(), "rows n .. npad are exact zeros"
        Ml = M[:, :n, :n].astype(LD)
        sum_bound("matvec n %d S %d" % (n, S), c[:, :n], Ml @ a.astype(LD), n, np.abs(Ml * a.astype(LD)).sum(2))


@pytest.mark.parametrize("S", [1, 10])
@pytest.mark.parametrize("n", [1, 129, 300])
def test_dots(n, S):
    rng = np.random.default_rng([2897, n, S])
    ldv = n + 7
    b, c = np.full((S, ldv), NAN), np.full((S, ldv), NAN)
    b[:, :n], c[:, :n] = rng.standard_normal((S, n)), rng.standard_normal((S, n))
    a = rng.standard_normal(n)
    d0 = np.full((S, S + 1), NAN)
    d = hessian.dots_check(b, c, a, ldv, n, S, d0, device=0).reshape(d0.shape)
    assert np.array_equal(bits(d), bits(hessian.dots_check(b, c, a, ldv, n, S, d0, device=0).reshape(d0.shape)))
    bl, cl, al = b[:, :n].astype(LD), c[:, :n].astype(LD), a.astype(LD)
    want, mag = np.zeros((S, S + 1), LD), np.zeros((S, S + 1))
    for s in range(S):
        for t in range(s, S):
            want[s, t], mag[s, t] = bl[s] @ cl[t], float(np.abs(bl[s] * cl[t]).sum())
        want[s, S], mag[s, S] = al @ cl[s], float(np.abs(al * cl[s]).sum())
    for s in range(S):
        assert not d[s, :s].any(), "zeros below the diagonal"
    sum_bound("dots n %d S %d" % (n, S), d, want, n, mag)


def traces_ref(M, K, n, pairs):
    Ml, Kl = M[:, :n, :n].astype(LD), K.astype(LD)
    want, mag = np.zeros(len(pairs), LD), np.zeros(len(pairs))
    for i, (sa, sb) in enumerate(pairs):
        T = (Kl if sa < 0 else Ml[sa]) * Ml[sb].T
        want[i], mag[i] = T.sum(), float(np.abs(T).sum())
    return want, mag


@pytest.mark.parametrize("n,npad,S,pairs", [
    (129, 192, 10, None),                       # the product's list at S = 10: 65 pairs, two launches
    (65, 192, 3, [(2, 1)]),                     # one pair
    (65, 128, 3, [(0, 2), (-1, 1), (1, 1)]),    # three
    (1030, 1088, 1, [(0, 0), (-1, 0)]),         # 289 tile partials per pair: the second round of hess_sum_kernel
    (1, 64, 2, [(-1, 0), (0, 1)]),
], ids=["S10-two-launches", "one-pair", "three-pairs", "289-partials", "n1"])
def test_traces(n, npad, S, pairs):
    pairs = R.trace_pairs(S) if pairs is None else pairs
    M, K, st, _ = given(n, npad, S, 2)
    nt = npad // 64
    part0, out0 = np.full(min(len(pairs), 64) * nt * nt, NAN), np.full(len(pairs), NAN)
    part, out = hessian.traces_check(M, S, st, n + 3, n, npad, pairs, part0, out0, device=0)
    part2, out2 = hessian.traces_check(M, S, st, n + 3, n, npad, pairs, part0, out0, device=0)
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(part), bits(part2))
    want, mag = traces_ref(M, K, n, pairs)
    sum_bound("traces n %d S %d, %d pairs" % (n, S, len(pairs)), out, want, n * n, mag)
    # the tiles' sums of the last launch add up to its traces
    last = len(pairs) - (len(pairs) - 1) // 64 * 64
    tiles = part.reshape(-1, nt * nt)[:last]
    assert np.isfinite(tiles).all()
    sum_bound("traces tiles", tiles.astype(LD).sum(1), want[len(pairs) - last:], n * n, mag[len(pairs) - last:])


@pytest.mark.parametrize("n", NS)
def test_quad(n):
    npad = npad_of(n, spare=n == 65)
    _, K, st, a = given(n, npad, 1, 3)
    ntl = (npad // 64) * (npad // 64 + 1) // 2
    part0, out0 = np.full(ntl * 4, NAN), np.full(4, NAN)
    part, out = hessian.quad_check(st, n + 3, a, n, npad, part0, out0, device=0)
    part2, out2 = hessian.quad_check(st, n + 3, a, n, npad, part0, out0, device=0)
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(part), bits(part2))
    Kl, al = K.astype(LD), a.astype(LD)
    aKa = np.outer(al, al) * Kl
    want = np.array([aKa.sum(), (Kl * Kl).sum(), al @ al, np.trace(Kl)])
    mag = np.array([np.abs(aKa).sum(), (Kl * Kl).sum(), al @ al, np.abs(np.diag(Kl)).sum()]).astype(F64)
    sum_bound("quad n %d" % n, out, want, n * (n + 1) // 2, mag)  # the stored pairs
    assert np.isfinite(part).all()
    sum_bound("quad tiles", part.reshape(ntl, 4).astype(LD).sum(0), want, n * (n + 1) // 2, mag)
