"""The kernel of Vecchia's approximation (gogp_amd/csrc/vecchia.hip) in isolation, through the hook gogp_test_vecchia on
caller-supplied parameters, rows, table and y, against the long-double reference of tests/vecchia_ref.py element by
element: the terms, the workgroups' values and their partial slot sums, every slot a quantity of its own.

Tolerance.  A running-error bound through a Cholesky factorisation and three substitutions is impractical, so every
quantity is held to 8 x the reference's own float64-minus-long-double difference (the factor of the CG tests): per
quantity the largest difference over the shapes of the case, relative to the quantity's largest magnitude, and a result
may differ from the long-double value by 8 x that share of the quantity's magnitude in its launch.  The blocks are well
conditioned (unit scale, noise variance 0.05, inputs uniform on a few length scales), so this is a statement about
rounding."""
import functools

import numpy as np
import pytest

import gram_ref as R
import grad_reduce_ref as G
import vecchia_ref as V
from cases import NAN64

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
NS = [1, 2, 65, 200]
MS = [0, 1, 7, 31, 32, 63]  # blocks of 1, 2, 8, 32 (one instance) and 33, 64 rows (the other)
DS = [1, 3, 8, 17]
FAMILIES = list(R.RADIAL) + ["periodic", "max_terms", "hyperpriors"]
CASES = [(k, D) for k in FAMILIES for D in DS] + [("ard", 3), ("ard", 8), ("ard", 17)]
NOISE_VAR = 0.05
FACTOR = 8.0
RATIOS = {}


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def kp_of(kind, D, noise_var=NOISE_VAR):
    return G.KP(D, R.terms_of(kind, D), noise_var=noise_var, dnoise=2 * noise_var)


@functools.lru_cache(maxsize=None)
def problem(D, N, m, seed=0):
    X, y, v = V.inputs(seed, N, D)
    t = V.random_table(np.random.default_rng([227, seed, N, m]), N, m, N)
    for a in (X, y, v, t):
        a.setflags(write=False)
    return X, y, v, t


def observe(gpm, kp, X, y, v, t, grad=True, max_blocks=0, want_terms=True):
    """Two launches with sentinels behind every array; returns (terms N x 3, partials blocks x NACC, vpart, value, info)."""
    N, D = X.shape
    m = t.shape[1]
    nb = gpm.vecchia_blocks(N, max_blocks)
    Xp, yp = np.concatenate([X.reshape(-1), np.full(2 * D, NAN64)]), np.concatenate([y, np.full(3, NAN64)])
    vp = None if v is None else np.concatenate([v, np.full(3, NAN64)])
    # behind the table: the index N, which no row may hold -- it names the NaN rows behind X, y and v, so a launch that
    # read a row too many would show NaN terms (and stay inside the buffers)
    tp = None if m == 0 else np.ascontiguousarray(np.concatenate([t.reshape(-1), np.full(2 * m, N, np.int32)]), dtype=np.int32)
    terms0 = np.full(3 * N + 4, NAN64) if want_terms else None
    part0 = np.full(nb * G.NACC + 4, NAN64) if grad else None
    vpart0 = np.full(nb + 2, NAN64)
    outs = [gpm.vecchia_check(kp.hook(gpm), Xp, yp, vp, N, tp, m, terms0, part0, vpart0, max_blocks=max_blocks)
            for _ in range(2)]
    a, b = outs
    for u, w in zip(a[:3], b[:3]):
        assert (u is None and w is None) or np.array_equal(bits(u), bits(w)), "two launches differ"
    assert bits(np.array([a[3]]))[0] == bits(np.array([b[3]]))[0] and a[4] == b[4], "two launches differ"
    terms, part, vpart, value, info = a
    if want_terms:
        assert np.array_equal(bits(terms[3 * N:]), bits(terms0[3 * N:])), "behind the terms"
    if grad:
        assert np.array_equal(bits(part[nb * G.NACC:]), bits(part0[nb * G.NACC:])), "behind the partials"
    assert np.array_equal(bits(vpart[nb:]), bits(vpart0[nb:])), "behind the values"
    return (terms[:3 * N].reshape(N, 3) if want_terms else None, part[:nb * G.NACC].reshape(nb, G.NACC) if grad else None,
            vpart[:nb], value, info)


def norm(ld, scale=None):
    """The magnitude a quantity of one launch is judged by: its largest element, or the one of `scale` where that is
    larger -- the forecast mu = y - L_qq z_q is an error in units of y even where it vanishes (no conditioning rows)."""
    mag = float(np.abs(ld).max()) if np.size(ld) else 0.0
    return mag if scale is None else max(mag, float(np.abs(scale).max()))


def rel_diff(f64, ld, scale=None):
    """max |f64 - ld| / norm of one quantity of one launch (0 where the quantity vanishes)."""
    mag = norm(ld, scale)
    return float(np.abs(np.asarray(f64, LD) - ld).max()) / mag if mag > 0 else 0.0


BASE = ("mu", "s", "logp", "vpart")
SLOTS = tuple("slot%d" % q for q in range(G.NACC))
QUANT = BASE + SLOTS  # every slot of the partial rows is a quantity of its own: their sizes differ by orders of magnitude


def quantities(ref):
    t = ref["terms"]
    out = dict(mu=t[:, 0], s=t[:, 1], logp=t[:, 2], vpart=ref["vpart"])
    out.update({"slot%d" % q: ref["partials"][:, q] for q in range(G.NACC)})
    return out


def device_quantities(terms, part, vpart):
    return quantities(dict(terms=terms, vpart=vpart, partials=part))


def shares_ok(share):
    """Every quantity but the slots no parameter owns (exact zeros on both sides) has a usable share."""
    return all(0 < share[q] < 1e-10 for q in BASE) and any(share[q] > 0 for q in SLOTS) and all(share[q] < 1e-10 for q in SLOTS)


@pytest.mark.parametrize("case", CASES, ids=["%s-D%d" % c for c in CASES])
def test_long_double(gpm, case):
    """Every N x m at the case's family and dimension: terms, workgroup values and partial slot sums element by element."""
    kind, D = case
    kp = kp_of(kind, D)
    runs, share = [], dict.fromkeys(QUANT, 0.0)
    for N in NS:
        for m in MS:
            X, y, v, t = problem(D, N, m)
            vv = v if (N + m) % 2 else None
            nb = gpm.vecchia_blocks(N)
            ld = quantities(V.observe(kp, X, y, vv, t, "ld", blocks=nb))
            f64 = quantities(V.observe(kp, X, y, vv, t, "f64", blocks=nb))
            for q in QUANT:
                share[q] = max(share[q], rel_diff(f64[q], ld[q], y if q == "mu" else None))
            runs.append((N, m, X, y, vv, t, ld))
    assert shares_ok(share), "the reference's own difference: %r" % share
    worst = 0.0
    for N, m, X, y, vv, t, ld in runs:
        terms, part, vpart, value, info = observe(gpm, kp, X, y, vv, t)
        assert info == 0, "N %d m %d: pivot" % (N, m)
        got = device_quantities(terms, part, vpart)
        for q in QUANT:
            assert np.isfinite(got[q]).all(), "%s N %d m %d" % (q, N, m)
            mag = norm(ld[q], y if q == "mu" else None)
            err = float(np.abs(got[q].astype(LD) - ld[q]).max())
            tol = FACTOR * share[q] * mag
            ratio = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
            worst = max(worst, ratio)
            assert err <= tol, "%s-D%d N %d m %d %s: |err| %.3g, allowed %.3g" % (kind, D, N, m, q, err, tol)
        owned = np.array([np.abs(ld[q]).max() > 0 for q in SLOTS])
        assert not part[:, ~owned].any(), "a slot no parameter owns is not zero"
        # the launch's value: the workgroups' values (each within its tolerance) summed in some fixed order of nb terms
        mag = float(np.abs(ld["vpart"]).sum())
        assert abs(value - float(ld["vpart"].sum())) <= (FACTOR * share["vpart"] * len(vpart) + G.gamma(len(vpart) + 1)) * mag
    RATIOS[case] = worst


def test_print_the_worst_ratios():
    by = {}
    for (kind, D), r in RATIOS.items():
        by[kind] = max(by.get(kind, 0.0), r)
    for kind, r in sorted(by.items()):
        print("vecchia kernel: worst |err| / allowed, %-12s %.3f" % (kind, r))


def test_waves_that_walk_several_targets(gpm):
    """A capped grid: 7 workgroups take 200 targets (m = 7 and 63), so a wave reuses its LDS and keeps its sums across ~29
    targets.  The terms keep the bits of the uncapped launch; the workgroups' values and every slot of the partial rows are
    held to the reference grouped the same way, the share of each the larger of the two shapes'."""
    kp = kp_of("max_terms", 3)
    runs, share = [], dict.fromkeys(QUANT, 0.0)
    for m in (7, 63):
        X, y, v, t = problem(3, 200, m)
        ld = quantities(V.observe(kp, X, y, v, t, "ld", blocks=7))
        f64 = quantities(V.observe(kp, X, y, v, t, "f64", blocks=7))
        for q in QUANT:
            share[q] = max(share[q], rel_diff(f64[q], ld[q], y if q == "mu" else None))
        runs.append((m, X, y, v, t, ld))
    assert shares_ok(share)
    for m, X, y, v, t, ld in runs:
        free = observe(gpm, kp, X, y, v, t)
        terms, part, vpart, value, info = observe(gpm, kp, X, y, v, t, max_blocks=7)
        assert info == 0 and part.shape == (7, G.NACC)
        assert np.array_equal(bits(terms), bits(free[0])), "a target's terms depend on the grid"
        got = device_quantities(terms, part, vpart)
        for q in ("vpart",) + SLOTS:
            tol = FACTOR * share[q] * norm(ld[q])
            err = float(np.abs(got[q].astype(LD) - ld[q]).max())
            assert err <= tol, "m %d %s: |err| %.3g, allowed %.3g" % (m, q, err, tol)


def test_sixty_four_dimensions(gpm):
    """D = 64, the largest, at m = 31 and 63 with full rows: with blocks of 64 rows the kernel's LDS passes 64 KB and the
    launch raises its limit.  The share of each quantity is the larger of the two shapes', as in test_long_double."""
    D, N = 64, 65
    kp = kp_of("matern52", D)
    runs, share = [], dict.fromkeys(QUANT, 0.0)
    for m in (31, 63):
        X, y, v, _ = problem(D, N, m)
        t = V.random_table(np.random.default_rng([239, m]), N, m, N, full=True)  # blocks of up to m + 1 rows
        ld = quantities(V.observe(kp, X, y, v, t, "ld", blocks=N))
        f64 = quantities(V.observe(kp, X, y, v, t, "f64", blocks=N))
        for q in QUANT:
            share[q] = max(share[q], rel_diff(f64[q], ld[q], y if q == "mu" else None))
        runs.append((m, X, y, v, t, ld))
    assert shares_ok(share)
    for m, X, y, v, t, ld in runs:
        terms, part, vpart, value, info = observe(gpm, kp, X, y, v, t)
        assert info == 0
        got = device_quantities(terms, part, vpart)
        for q in QUANT:
            tol = FACTOR * share[q] * norm(ld[q], y if q == "mu" else None)
            err = float(np.abs(got[q].astype(LD) - ld[q]).max())
            if tol > 0:
                print("D 64 m %d %s: |err| %.3g, allowed %.3g" % (m, q, err, tol))
            assert err <= tol, "D 64 m %d %s: |err| %.3g, allowed %.3g" % (m, q, err, tol)


def test_value_pass_alone(gpm):
    """Without the gradient's pass (no partials) and without terms the value and the workgroups' values keep their bits."""
    kp = kp_of("matern52", 3)
    X, y, v, t = problem(3, 65, 31)
    full = observe(gpm, kp, X, y, v, t)
    alone = observe(gpm, kp, X, y, v, t, grad=False, want_terms=False)
    assert alone[0] is None and alone[1] is None
    assert np.array_equal(bits(alone[2]), bits(full[2])) and alone[3] == full[3] and alone[4] == 0


@pytest.mark.parametrize("m", [7, 31, 32, 63])
def test_a_target_alone_has_the_bits_it_has_in_a_launch(gpm, m):
    """Target i of a launch of 200 against a launch that holds its block alone, its rows renumbered in the table's order."""
    kp = kp_of("hyperpriors", 3)
    X, y, v, t = problem(3, 200, m)
    terms = observe(gpm, kp, X, y, v, t)[0]
    for i in (1, 64, 137, 199):
        c = V.rows_of(t, i)
        b = np.concatenate([c, [i]])
        q = len(c)
        t1 = np.full((q + 1, m), -1, np.int32)
        t1[q, :q] = np.arange(q)
        alone = observe(gpm, kp, np.ascontiguousarray(X[b]), np.ascontiguousarray(y[b]), np.ascontiguousarray(v[b]), t1)[0]
        assert np.array_equal(bits(alone[q]), bits(terms[i])), "target %d (q = %d)" % (i, q)


def test_both_instances_give_a_target_the_same_bits(gpm):
    """The table of m = 7 padded to 63 columns runs on the 64-row instance: same terms, same partial rows."""
    kp = kp_of("matern32", 3)
    X, y, v, t = problem(3, 65, 7)
    wide = np.full((65, 63), -1, np.int32)
    wide[:, :7] = t
    a, b = observe(gpm, kp, X, y, v, t), observe(gpm, kp, X, y, v, wide)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_indefinite_block_reports_the_lowest_target(gpm):
    """Rows 5 and 9 coincide and there is no noise: with the Normal kernel at scale 1 the blocks [5, 9] and [5, 9, 20] are
    [[1, 1], [1, 1]] in exact arithmetic on the device too, so their second pivot is exactly 0.  The launch reports target
    9, the two targets hold NaN, and every other target keeps the bits of the launch whose table leaves 9 and 20 alone."""
    D, N, m = 2, 40, 3
    kp = G.KP(D, [dict(kind=R.K_NORMAL, c=1.0, inv_len=0.5)], noise_var=0.0)
    X, y, _ = V.inputs(3, N, D)
    X = X.copy()
    X[9] = X[5]
    t = V.random_table(np.random.default_rng(229), N, m, N)
    t[9], t[20] = (5, -1, -1), (5, 9, -1)
    for i in range(N):  # no other block holds both rows
        if i not in (9, 20) and 5 in t[i] and 9 in t[i]:
            t[i] = -1
    ok = t.copy()
    ok[9] = ok[20] = -1
    terms, part, vpart, value, info = observe(gpm, kp, X, y, None, t)
    base = observe(gpm, kp, X, y, None, ok)
    assert info == 10 and base[4] == 0
    assert np.isnan(terms[[9, 20]]).all()
    keep = np.ones(N, bool)
    keep[[9, 20]] = False
    assert np.array_equal(bits(terms[keep]), bits(base[0][keep])), "another target's terms moved"
    assert np.array_equal(bits(vpart[keep]), bits(base[2][keep])) and vpart[9] == 0.0 and vpart[20] == 0.0
    assert np.array_equal(bits(part[keep]), bits(base[1][keep])) and not part[[9, 20]].any()
    ref = V.observe(kp, X, y, None, t, "ld", blocks=N)
    assert ref["failed"] == [9, 20]


@pytest.mark.parametrize("kind", FAMILIES + ["ard"])
def test_produce(gpm, kind):
    """mu and sigma of 1 and 65 test points on random tables of every m, against the long-double reference."""
    D, N = 3, 65
    kp = kp_of(kind, D)
    share, runs = dict(mu=0.0, sigma=0.0), []
    for mz in (1, 65):
        for m in MS:
            X, y, v, _ = problem(D, N, m)
            rng = np.random.default_rng([233, mz, m])
            Z = rng.uniform(-3.0, 3.0, (mz, D))
            tz = V.random_table(rng, mz, m, N, causal=False)
            vv = v if m % 2 else None
            ld, f64 = V.produce(kp, X, y, vv, Z, tz, "ld"), V.produce(kp, X, y, vv, Z, tz, "f64")
            share["mu"] = max(share["mu"], rel_diff(f64[0], ld[0], y))
            share["sigma"] = max(share["sigma"], rel_diff(f64[1], ld[1]))
            runs.append((mz, m, X, y, vv, Z, tz, ld))
    assert 0 < share["mu"] < 1e-10 and 0 < share["sigma"] < 1e-10
    for mz, m, X, y, vv, Z, tz, ld in runs:
        Xp, yp = np.concatenate([X.reshape(-1), np.full(2 * D, NAN64)]), np.concatenate([y, np.full(3, NAN64)])
        vp = None if vv is None else np.concatenate([vv, np.full(3, NAN64)])
        Zp = np.concatenate([Z.reshape(-1), np.full(D, NAN64)])
        tp = None if m == 0 else np.ascontiguousarray(tz.reshape(-1))
        out0 = np.full(2 * mz + 3, NAN64)
        a = gpm.vecchia_check(kp.hook(gpm), Xp, yp, vp, N, tp, m, out0, Z=Zp, targets=mz)
        b = gpm.vecchia_check(kp.hook(gpm), Xp, yp, vp, N, tp, m, out0, Z=Zp, targets=mz)
        assert np.array_equal(bits(a[0]), bits(b[0])) and a[4] == b[4] == 0
        assert np.array_equal(bits(a[0][2 * mz:]), bits(out0[2 * mz:])), "behind mu and sigma"
        for q, got, want in (("mu", a[0][:mz], ld[0]), ("sigma", a[0][mz:2 * mz], ld[1])):
            tol = FACTOR * share[q] * norm(want, y if q == "mu" else None)
            err = float(np.abs(got.astype(LD) - want).max())
            assert err <= tol, "%s mz %d m %d %s: |err| %.3g, allowed %.3g" % (kind, mz, m, q, err, tol)


def test_hook_refuses_bad_arguments(gpm):
    kp = kp_of("normal", 2)
    X, y, v, t = problem(2, 8, 3)
    bad = t.copy()
    bad[3, 0] = 3  # not causal
    from gogp_amd.gp import GogpError
    for table, n in ((bad, 8), (t, 9)):
        with pytest.raises(GogpError):
            gpm.vecchia_check(kp.hook(gpm), X.reshape(-1).copy(), y.copy(), None, n, np.ascontiguousarray(table.reshape(-1)), 3,
                              np.zeros(3 * n), None, np.zeros(n))
