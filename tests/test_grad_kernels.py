"""The kernels that turn K^-1 into the gradient, in isolation (run with -m gpu on the MI355X box): grad_reduce_kernel,
grad_final_kernel, mirror_lower_kernel and xgrad_kernel of grad.hip and grad_ard_mfma_kernel of grad_mfma.hip, every
instance through the launchers' own selection (the case names it), double and float K^-1.

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h.  tests/grad_reduce_ref.py holds
the references and the model of the bound:
- "ld": random full-mantissa operands -- K^-1 with no symmetry and no relation to X, alpha random -- against long-double
  sums, |got - ref| <= e_q per slot with the running bound of an fp64 evaluation in any order, no case-specific factor;
- "exact": identical inputs, integer alpha and K^-1, c a power of two: the sums are integers and come back BIT FOR BIT.
  This pins which elements are read with which weight (masks at ragged n, the tile walk, the upper tiles a rank skips,
  candidates);
- sentinels (NaNs with a payload): every element of K^-1 above the diagonal, its rows and columns >= n, alpha[n:], the
  rows n .. npad - 1 of X, `partials` and `out` before the launch.  One exception, the contract stated at
  launch_grad_reduce (common.h): the one-radial-term ARD instances multiply the coordinates that FOLLOW a live row's
  own by inv_len = 0, so for them the rows >= n of X hold a large finite number instead (the product zero-fills them).
Two launches of every case must agree bit for bit, rows 0 .. blocks - 1 of `partials` must be finite, and the slots of
dimensions >= D and of terms and periods the kernel lacks must be exactly 0.

The largest |got - ref| / e_q per instance family is printed by the last test (-s shows it).
"""
import functools

import numpy as np
import pytest

import grad_reduce_ref as R
from cases import NAN32, NAN64

pytestmark = pytest.mark.gpu

NACC, TRACE, ARD0 = R.NACC, R.ACC_TRACE, R.ACC_ARD0
FINITE_PAD = 2.0 ** 100
RATIOS = {}


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def nan_of(dt):
    return NAN64 if dt == np.float64 else NAN32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))


# ---- kernels -----------------------------------------------------------------------------------------------------------
def _il(D, seed):
    return np.random.default_rng(900 + seed).uniform(0.6, 1.4, D) / np.sqrt(D)


def radial(D, kind=R.K_NORMAL, ard=False, c=1.3):
    return R.KP(D, [dict(kind=kind, ard=ard, c=c, inv_len=_il(D, D) if ard else 0.9 / np.sqrt(D))])


def two_term(D):
    return R.KP(D, [dict(kind=R.K_NORMAL, ard=True, c=0.8, inv_len=_il(D, D + 1)),
                    dict(kind=R.K_MATERN32, c=1.1, inv_len=0.7 / np.sqrt(D))])


def hyperpriors():  # tests/cases.py: c1 Matern52(l1) + c2 Periodic(l2, 10 p)
    return R.KP(1, [dict(kind=R.K_MATERN52, c=1.0, inv_len=1 / 0.5),
                    dict(kind=R.K_PERIODIC, c=0.6, inv_len=1 / 1.3, w=np.pi / (10.0 * 0.05))])


def max_terms():
    return R.KP(2, [dict(kind=R.K_NORMAL, c=0.7, inv_len=1.1), dict(kind=R.K_MATERN32, c=1.2, inv_len=0.8),
                    dict(kind=R.K_MATERN52_TEXTBOOK, c=0.4, inv_len=1.7), dict(kind=R.K_PERIODIC, c=0.9, inv_len=0.6, w=4.1)])


def with_events(kp, nev, axis):
    b = np.linspace(0.05, 0.95, 2 * nev)
    ev = [(b[2 * e], b[2 * e + 1], 0.3 + 0.5 * e / max(nev - 1, 1)) for e in range(nev)][::-1]  # not in coordinate order
    return R.KP(kp.ndim, kp.terms, events=ev, ev_axis=axis)


def live_slots(kp):
    s = {TRACE}
    for t, T in enumerate(kp.terms):
        s.add(3 * t)
        if not T["ard"]:
            s.add(3 * t + 1)
        if T["kind"] == R.K_PERIODIC:
            s.add(3 * t + 2)
        if T["ard"]:
            s.update(range(ARD0, ARD0 + kp.ndim))
    return sorted(s)


def scalar_instance(kp, mfma_min, ev):
    """What launch_grad_reduce selects, as the case's name."""
    a = kp.ard_dims
    if ev:
        return "ev/radial1" if kp.radial1 else "ev/generic"
    if kp.radial1 and a and a >= mfma_min:
        return "mfma%d" % ((a + 15) // 16 * 16)
    if a <= 8:
        return ("scalar%d" % (8 if a else 0)) if kp.radial1 else ("generic%d" % (8 if a else 0))
    if kp.radial1 and a > 16:
        return "scalar" + "+".join(str(8 if a - a0 <= 8 else 16 if a - a0 <= 16 else 32) for a0 in range(0, a, 32))
    return ("scalar" if kp.radial1 else "generic") + "+".join("16" for _ in range(0, a, 16))


def family_of(inst):
    if inst.startswith(("mfma", "ev", "generic")):
        return "generic" if inst.startswith("generic") else "events" if inst.startswith("ev") else inst
    return "scalar" + inst[6:].split("+")[0]


# ---- operands ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(mode, npad, n, D, seed=0, offset=0.0, boundary=None):
    rng = np.random.default_rng(1000 * seed + 7 * npad + n + D)
    if mode == "exact":
        X = np.tile(rng.uniform(0, 1, (1, D)), (n, 1))
        alpha = rng.integers(-4, 5, n).astype(float)
        K = rng.integers(-8, 9, (npad, npad)).astype(float)
    else:
        X = rng.uniform(0, 1, (n, D)) + offset
        if boundary is not None:  # points exactly on event boundaries
            axis, vals = boundary
            X[:len(vals), axis] = vals
        alpha = rng.normal(size=n)
        K = rng.normal(size=(npad, npad))
    for a in (X, alpha, K):
        a.setflags(write=False)
    return X, alpha, K


def flat_x(X, n, npad, finite_pad):
    D = X.shape[1]
    out = np.zeros(npad * D + R.MAX_NDIM)   # the slack stays zero
    out[:n * D] = X.ravel()
    out[n * D:npad * D] = FINITE_PAD if finite_pad else NAN64
    return out


def flat_alpha(alpha, n, npad):
    out = np.full(npad, NAN64)
    out[:n] = alpha
    return out


def flat_kinv(K, n, rows, cols, ld, dt):
    """rows x cols (global indices of the local rows / columns) of K as a launch sees them: the elements i < n, j <= i,
    sentinels everywhere else -- above the diagonal, rows and columns >= n, the columns up to ld."""
    out = np.full((len(rows), ld), nan_of(dt), dt)
    live = (rows[:, None] < n) & (cols[None, :] <= rows[:, None])
    sub = K[np.ix_(rows, cols)].astype(dt)
    out[:, :len(cols)][live] = sub[live]
    return out.ravel()


def finite_pad_of(kp, mfma_min):
    return bool(kp.radial1 and kp.ard_dims and kp.ard_dims < mfma_min)


def launch(gpm, kp, Xf, af, Kf, ld, n, npad, mfma_min, ev, max_blocks, local=None, device=-1):
    """Two launches on sentinel-filled partials / out: (out, blocks) after asserting bit-identical runs, finite rows
    0 .. blocks - 1 of partials and an untouched tail."""
    if local is None:
        blocks = gpm.grad_blocks(npad, max_blocks)
    else:
        mrows, ncols, grid = local
        blocks = gpm.grad_blocks(npad, max_blocks, mrows, ncols)
    part, out = np.full(blocks * NACC + 5, NAN64), np.full(NACC, NAN64)
    res = []
    for _ in range(2):
        if local is None:
            p, o = gpm.grad_reduce_check(kp.hook(gpm), Xf, af, Kf, ld, n, npad, part, out, kp.ard_dims, kp.radial1, mfma_min,
                                         ev, max_blocks, device=device)
            o = o[0]
        else:
            p, o = gpm.grad_reduce_local_check(kp.hook(gpm), Xf, af, Kf, ld, n, npad, mrows, ncols, grid, part, out,
                                               kp.ard_dims, kp.radial1, mfma_min, ev, max_blocks, device=device)
        res.append((p, o))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), "two runs differ"
    p, o = res[0]
    assert np.isfinite(p[:blocks * NACC]).all(), "partials rows 0 .. blocks - 1"
    assert same_bits(p[blocks * NACC:], part[blocks * NACC:]), "partials beyond the launch's rows"
    return o, blocks


def check_ld(kp, got, ref, bnd, families, what):
    live = live_slots(kp)
    dead = [q for q in range(NACC) if q not in live]
    assert np.all(bits(got[dead]) == 0), "%s: dead slots %s" % (what, [q for q in dead if bits(got[q:q + 1])[0]])
    err = np.abs(got[live].astype(R.LD) - ref[live]).astype(np.float64)
    b = bnd[live]
    pos = b > 0   # (a slot whose every term is exactly 0 -- one point, s = 0 -- has bound 0 and must be exact)
    # gamma_m sum |T| with m <= 2^18 pairs of random sign is some 2^18 2^-53 2^9 = 1.5e-8 of the sum itself; 64 times that
    # for a sum that happens to cancel further
    assert np.all(err[~pos] == 0) and b.max() <= 1e-6 * np.abs(ref[live]).astype(np.float64).max(), \
        "%s: the bound is vacuous" % what
    ratio = np.divide(err, b, out=np.zeros_like(err), where=pos)
    print("RATIO %-40s %.3f" % (what, ratio.max()))
    for f in families:
        note(f, ratio.max())
    bad = [(live[i], float(got[live[i]]), float(ref[live[i]]), float(ratio[i])) for i in np.where(ratio > 1)[0]]
    assert not bad, "%s: (slot, got, ref, |got - ref| / e_q) %s" % (what, bad)


def check_exact(got, want, what):
    assert np.array_equal(got, want), "%s: slots %s got %s want %s" % (
        what, np.where(got != want)[0], got[got != want], want[got != want])


@functools.lru_cache(maxsize=None)
def global_ref(kpk, npad, n, form, seed=0, offset=0.0, boundary=None):
    kp = KPS[kpk]()
    X, alpha, K = operands("ld", npad, n, kp.ndim, seed, offset, boundary)
    Ks = [K[:n, :n], K[:n, :n].astype(np.float32)]
    return R.slot_sums(kp, X, n, alpha, Ks, form=form)


def run_global(gpm, kpk, npad, n, mfma_min=65, ev=False, max_blocks=(0, 3, 1), precs=(64, 32), modes=("ld", "exact"),
               seed=0, offset=0.0, boundary=None):
    kp = KPS[kpk]()
    inst = scalar_instance(kp, mfma_min, ev)
    form = "mfma" if inst.startswith("mfma") else "diff"
    ld = npad + 2
    idx = np.arange(npad)
    for mode in modes:
        X, alpha, K = operands(mode, npad, n, kp.ndim, seed, offset, boundary)
        kpm = kp
        if mode == "exact":
            kpm = R.KP(kp.ndim, [dict(T, c=2.0 ** (t - 1)) for t, T in enumerate(kp.terms)], kp.events, kp.ev_axis)
        else:
            ref, bnd = global_ref(kpk, npad, n, form, seed, offset, boundary)
        Xf, af = flat_x(X, n, npad, finite_pad_of(kp, mfma_min)), flat_alpha(alpha, n, npad)
        for prec in precs:
            dt = np.float64 if prec == 64 else np.float32
            Kf = flat_kinv(K, n, idx, idx, ld, dt)
            for mb in max_blocks:
                what = "%s %s n=%d/%d f%d mb=%d %s" % (kpk, inst, n, npad, prec, mb, mode)
                got, _ = launch(gpm, kpm, Xf, af, Kf, ld, n, npad, mfma_min, ev, mb)
                if mode == "exact":
                    check_exact(got, R.exact_slots(kpm, alpha, K, n), what)
                else:
                    check_ld(kp, got, ref[int(prec == 32)], bnd[int(prec == 32)], [family_of(inst)] + (["float"] if prec == 32 else []),
                             what)


SCALAR_D = [0, 5, 8, 9, 16, 17, 24, 33, 40, 41, 48, 49, 64]
MFMA_D = [2, 16, 17, 32, 33, 48, 49, 64]
TWO_D = [5, 16, 17, 33, 64]
KINDS = {"normal": R.K_NORMAL, "matern32": R.K_MATERN32, "matern52": R.K_MATERN52, "matern52t": R.K_MATERN52_TEXTBOOK}
KPS = {"hyperpriors": hyperpriors, "max_terms": max_terms,
       "periodic": lambda: R.KP(2, [dict(kind=R.K_PERIODIC, c=1.2, inv_len=0.8, w=np.pi / 0.45)])}
for _d in SCALAR_D:
    KPS["ard%d" % _d] = functools.partial(radial, _d or 3, R.K_NORMAL, _d > 0)
for _d in MFMA_D:
    KPS["ard%d" % _d] = functools.partial(radial, _d, R.K_NORMAL, True)
    KPS["ardm%d" % _d] = functools.partial(radial, _d, R.K_MATERN52, True)
for _d in TWO_D:
    KPS["two%d" % _d] = functools.partial(two_term, _d)
for _k, _v in KINDS.items():
    KPS[_k] = functools.partial(radial, 3, _v)
for _nev in (1, 3, R.MAX_EVENTS):
    KPS["ev%d" % _nev] = functools.partial(lambda nev: with_events(radial(2, R.K_MATERN52), nev, 1), _nev)
    KPS["evg%d" % _nev] = functools.partial(lambda nev: with_events(hyperpriors_2d(), nev, 1), _nev)


def hyperpriors_2d():
    return R.KP(2, [dict(kind=R.K_MATERN52, c=1.0, inv_len=1.4), dict(kind=R.K_PERIODIC, c=0.6, inv_len=0.9, w=5.0)])


#: (npad, n): ragged and full, one tile row wholly beyond n (130 in 256), one point, one tile
SHAPES = [(256, 1), (256, 64), (256, 130), (256, 255), (256, 256), (512, 449), (512, 512)]
INSTANCE_SHAPE = (256, 191)   # three live tile rows, the fourth beyond n; max_blocks 3: workgroups walk 4, 3, 3 tiles


@pytest.mark.parametrize("npad,n", SHAPES)
@pytest.mark.parametrize("kpk,mfma_min", [("ard0", 65), ("ard5", 65), ("ard17", 65), ("ard17", 1), ("two5", 65), ("hyperpriors", 65)])
def test_shapes(gpm, kpk, mfma_min, npad, n):
    """Every shape x max_blocks (workgroups that walk 1, several, all tiles) on one instance of each kernel form."""
    run_global(gpm, kpk, npad, n, mfma_min)


@pytest.mark.parametrize("D", SCALAR_D)
def test_scalar_radial_instances(gpm, D):
    """One radial term on the scalar rows: instances 0 / 8 / 16 / 32 and last passes of 8, 16 and 32."""
    run_global(gpm, "ard%d" % D, *INSTANCE_SHAPE, mfma_min=65, max_blocks=(3,))


@pytest.mark.parametrize("D", TWO_D)
def test_two_term_ard_passes_of_16(gpm, D):
    run_global(gpm, "two%d" % D, *INSTANCE_SHAPE, max_blocks=(3,))


@pytest.mark.parametrize("kpk", list(KINDS) + ["periodic", "hyperpriors", "max_terms"])
def test_non_ard_kinds(gpm, kpk):
    run_global(gpm, kpk, *INSTANCE_SHAPE, max_blocks=(3,))


@pytest.mark.parametrize("D", MFMA_D)
@pytest.mark.parametrize("kind", ["ard", "ardm"])
def test_matrix_core_instances(gpm, kind, D):
    run_global(gpm, "%s%d" % (kind, D), *INSTANCE_SHAPE, mfma_min=1, max_blocks=(3,))


def test_matrix_core_offset_inputs(gpm):
    """Inputs that carry an offset of 2^20 per coordinate: the bound is computed on the centred form, so a kernel that
    does not centre each tile misses it by orders of magnitude."""
    run_global(gpm, "ard17", *INSTANCE_SHAPE, mfma_min=1, max_blocks=(3,), modes=("ld",), offset=2.0 ** 20)


@pytest.mark.parametrize("nev", [1, 3, R.MAX_EVENTS])
@pytest.mark.parametrize("kpk", ["ev", "evg"])
def test_events(gpm, kpk, nev):
    """Event discounts with and without radial1, on coordinate 1, with points exactly on `from` / `to` boundaries."""
    kp = KPS["%s%d" % (kpk, nev)]()
    vals = tuple(v for e in kp.events[:4] for v in e[:2])
    run_global(gpm, "%s%d" % (kpk, nev), *INSTANCE_SHAPE, ev=True, max_blocks=(3,), boundary=(1, vals))


@pytest.mark.parametrize("kpk,mfma_min", [("ard17", 65), ("ard17", 1)])
def test_candidates(gpm, kpk, mfma_min):
    """k = 3 candidates on gridDim.z: parameters, alpha, K^-1, partials and out per candidate, X shared."""
    npad, n = INSTANCE_SHAPE
    k, ld = 3, npad
    base = KPS[kpk]()
    bstride = npad * ld + 512
    form = "mfma" if mfma_min == 1 else "diff"
    for mode in ("ld", "exact"):
        X = operands(mode, npad, n, base.ndim)[0]
        kps, al, Ks = [], [], []
        for c in range(k):
            T = base.terms[0]
            kps.append(R.KP(base.ndim, [dict(T, c=2.0 ** c if mode == "exact" else T["c"] * (1 + 0.2 * c),
                                             inv_len=T["inv_len"] * (1 + 0.1 * c))]))
            _, a, K = operands(mode, npad, n, base.ndim, seed=20 + c)
            al.append(a)
            Ks.append(K)
        blocks = gpm.grad_blocks(npad, 3)
        af, Kf = np.full((k - 1) * bstride + npad, NAN64), np.full((k - 1) * bstride + npad * ld, NAN64)
        for c in range(k):
            af[c * bstride:c * bstride + npad] = flat_alpha(al[c], n, npad)
            Kf[c * bstride:c * bstride + npad * ld] = flat_kinv(Ks[c], n, np.arange(npad), np.arange(npad), ld, np.float64)
        part, out = np.full((k - 1) * bstride + blocks * NACC, NAN64), np.full(k * NACC, NAN64)
        Xf = flat_x(X, n, npad, finite_pad_of(base, mfma_min))
        p, o = gpm.grad_reduce_check([q.hook(gpm) for q in kps], Xf, af, Kf, ld, n, npad, part, out, base.ndim, True, mfma_min,
                                     False, 3, bstride)
        for c in range(k):
            assert np.isfinite(p[c * bstride:c * bstride + blocks * NACC]).all()
            if c + 1 < k:
                assert same_bits(p[c * bstride + blocks * NACC:(c + 1) * bstride], part[c * bstride + blocks * NACC:(c + 1) * bstride])
            what = "candidate %d %s %s" % (c, kpk, form)
            if mode == "exact":
                check_exact(o[c], R.exact_slots(kps[c], al[c], Ks[c], n), what)
            else:
                ref, bnd = R.slot_sums(kps[c], X, n, al[c], [Ks[c][:n, :n]], form=form)
                check_ld(kps[c], o[c], ref[0], bnd[0], ["mfma32" if mfma_min == 1 else "scalar32"], what)


def test_final_kernel_strided_loop(gpm):
    """grad_final_kernel sums `blocks` partial rows with 256 threads: more than 256 blocks make its loop stride."""
    nt = 1
    while nt * (nt + 1) // 2 <= 256:
        nt += 1
    npad, n = 64 * nt, 64 * nt - 37
    assert gpm.grad_blocks(npad) == nt * (nt + 1) // 2 > 256
    run_global(gpm, "matern32", npad, n, max_blocks=(0,), precs=(64,), modes=("exact",))


# ---- the local tiles of a 2-D block-cyclic K^-1 -----------------------------------------------------------------------------
NB = 512


def rank_indices(nblk, P, p):
    b = np.arange(nblk)[np.arange(nblk) % P == p]
    return (b[:, None] * NB + np.arange(NB)[None, :]).ravel()


def run_local(gpm, kpk, Pr, Pc, mult, mode, mfma_min=65, ev=False, prec=64, max_blocks=0):
    kp = KPS[kpk]()
    nblk = max(Pr, Pc) * mult
    npad = NB * nblk
    n = npad - 211   # ragged inside the last block
    X, alpha, K = operands(mode, npad, n, kp.ndim, seed=3)
    if mode == "exact":
        kp = R.KP(kp.ndim, [dict(T, c=2.0 ** (t - 1)) for t, T in enumerate(kp.terms)], kp.events, kp.ev_axis)
    inst = scalar_instance(kp, mfma_min, ev)
    form = "mfma" if inst.startswith("mfma") else "diff"
    Xf, af = flat_x(X, n, npad, finite_pad_of(kp, mfma_min)), flat_alpha(alpha, n, npad)
    dt = np.float64 if prec == 64 else np.float32
    total = np.zeros(NACC)
    for pr in range(Pr):
        for pc in range(Pc):
            rows, cols = rank_indices(nblk, Pr, pr), rank_indices(nblk, Pc, pc)
            ld = len(cols) + 2
            Kf = flat_kinv(K, n, rows, cols, ld, dt)
            what = "local %s %s rank (%d,%d) of %dx%d x%d f%d %s" % (kpk, inst, pr, pc, Pr, Pc, mult, prec, mode)
            got, _ = launch(gpm, kp, Xf, af, Kf, ld, n, npad, mfma_min, ev, max_blocks,
                            local=(len(rows), len(cols), (pr, Pr, pc, Pc)))
            if mode == "exact":
                check_exact(got, R.exact_slots(kp, alpha, K, n, R.tile_mask(n, (pr, Pr, pc, Pc), NB)), what)
                total += got
            else:
                r, c = rows[rows < n], cols[cols < n]
                Ksub = K[np.ix_(r, c)]
                ref, bnd = R.slot_sums(kp, X, n, alpha, [Ksub.astype(dt)], rows=r, cols=c, form=form)
                if (c[None, :] <= r[:, None]).any():
                    check_ld(kp, got, ref[0], bnd[0], ["local"] + (["float"] if prec == 32 else []), what)
                else:  # a rank with nothing below the diagonal
                    assert np.all(bits(got) == 0), what
    if mode == "exact":
        check_exact(total, R.exact_slots(kp, alpha, K, n), "the ranks' sums add up to the global one")


GRIDS = [(1, 2), (2, 2), (2, 3)]


@pytest.mark.parametrize("Pr,Pc", GRIDS)
@pytest.mark.parametrize("kpk,mfma_min,ev", [("ard0", 65, False), ("ard17", 65, False), ("ard17", 1, False),
                                             ("two5", 65, False), ("ev3", 65, True)])
def test_local_exact(gpm, kpk, mfma_min, ev, Pr, Pc):
    """Every rank of every grid, one and two distribution blocks per rank and dimension; workgroups that walk one tile
    and several; the ranks' sums add up to the global one."""
    for mult, mb, prec in ((1, 0, 64), (2, 7, 32)):
        run_local(gpm, kpk, Pr, Pc, mult, "exact", mfma_min, ev, prec, mb)


@pytest.mark.parametrize("Pr,Pc", GRIDS)
@pytest.mark.parametrize("kpk,mfma_min,ev,prec", [("ard0", 65, False, 64), ("ard17", 65, False, 32), ("ard17", 1, False, 64),
                                                  ("two5", 65, False, 64), ("ev3", 65, True, 32)])
def test_local_ld(gpm, kpk, mfma_min, ev, prec, Pr, Pc):
    run_local(gpm, kpk, Pr, Pc, 1, "ld", mfma_min, ev, prec, 5)


# ---- the dynamic-LDS limit is per device ----------------------------------------------------------------------------------
def test_large_lds_instance_on_every_device(gpm):
    """Radial D = 64 on the scalar rows (instance 32, 77 KB of dynamic LDS): the limit is raised per launch, because the
    attribute belongs to the function on the current device -- the launch on device 1 comes AFTER the one on device 0."""
    import torch
    kp = KPS["ard64"]()
    npad, n = 256, 130
    X, alpha, K = operands("ld", npad, n, 64)
    ref, bnd = global_ref("ard64", npad, n, "diff")
    Xf, af = flat_x(X, n, npad, True), flat_alpha(alpha, n, npad)
    Kf = flat_kinv(K, n, np.arange(npad), np.arange(npad), npad, np.float64)
    for dev in range(min(2, torch.cuda.device_count())):   # one GPU: the first half only
        got, _ = launch(gpm, kp, Xf, af, Kf, npad, n, npad, 65, False, 0, device=dev)
        check_ld(kp, got, ref[0], bnd[0], ["scalar32"], "ard64 on device %d" % dev)


# ---- the input gradient -------------------------------------------------------------------------------------------------
def xgrad_kinv(K, n, npad, ld):
    """K^-1 as launch_xgrad gets it: the lower triangle, the diagonal 32 x 32 blocks symmetric (the product's LAUUM leaves
    them full; mirror_lower_kernel skips them), sentinels elsewhere above the diagonal, in rows / columns >= n and up to ld."""
    out = np.full((npad, ld), NAN64)
    i, j = np.arange(npad)[:, None], np.arange(npad)[None, :]
    low = (j <= i) & (i < n)
    out[:, :npad][low] = K[low]
    blk = (i // 32 == j // 32) & (j > i) & (j < n)
    out[:, :npad][blk] = K.T[blk]
    return out.ravel()


def run_xgrad(gpm, kp, npad, n, ev, family, what, boundary=None):
    D = kp.ndim
    X, alpha, K = operands("ld", npad, n, D, seed=5, boundary=boundary)
    ld = npad + 4
    Kf = xgrad_kinv(K, n, npad, ld)
    gx0 = np.full(npad * D, NAN64)
    Xf = flat_x(X, n, npad, False)[:npad * D]
    Ka, gx = gpm.xgrad_check(kp.hook(gpm), Xf, flat_alpha(alpha, n, npad), Kf, ld, n, npad, gx0, ev)
    Ka2, gx2 = gpm.xgrad_check(kp.hook(gpm), Xf, flat_alpha(alpha, n, npad), Kf, ld, n, npad, gx0, ev)
    assert same_bits(Ka, Ka2) and same_bits(gx, gx2), "two runs differ"
    A, B = Ka.reshape(npad, ld), Kf.reshape(npad, ld)
    low = np.tril(np.ones((npad, npad), bool))
    assert same_bits(A[:, :npad][low], B[:, :npad][low]), "the lower triangle changed"
    assert same_bits(A[:, npad:], B[:, npad:]), "columns beyond npad changed"
    assert same_bits(A[:, :npad].T[low], A[:, :npad][low]), "upper triangle != transpose of the lower"
    gx = gx.reshape(npad, D)
    assert same_bits(gx[n:], gx0.reshape(npad, D)[n:]), "rows >= n of gx were written"
    Ks = np.tril(K[:n, :n]) + np.tril(K[:n, :n], -1).T
    ref, bnd = R.xgrad_sums(kp, X, n, alpha, Ks)
    err = np.abs(gx[:n].astype(R.LD) - ref).astype(np.float64)
    pos = bnd > 0
    assert np.all(err[~pos] == 0) and bnd.max() <= 1e-6 * np.abs(ref).astype(np.float64).max()
    ratio = np.divide(err, bnd, out=np.zeros_like(err), where=pos)
    print("RATIO %-40s %.3f" % (what, ratio.max()))
    note(family, ratio.max())
    assert ratio.max() <= 1, "%s: worst (i, d) %s ratio %.3g" % (what, np.unravel_index(ratio.argmax(), ratio.shape),
                                                                 ratio.max())


def xgrad_family(D, ev):
    if ev:
        return "xgrad ev %d" % (4 if D <= 4 else 8 if D <= 8 else 16)
    return "xgrad %d" % (4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32)


@pytest.mark.parametrize("D", [1, 4, 5, 8, 9, 16, 17, 32, 33, 45, 64])
def test_xgrad_radial(gpm, D):
    """Instances 4 / 8 / 16 / 32 and two passes of 32; D = 45 and 64 need more than 64 KB of dynamic LDS."""
    run_xgrad(gpm, radial(D, R.K_MATERN52, ard=D > 1), 256, 191, False, xgrad_family(D, False), "xgrad radial D=%d" % D)


@pytest.mark.parametrize("D", [3, 8, 9, 17, 33])
def test_xgrad_events(gpm, D):
    """The event instances: 4 / 8 / 16 and passes of 16, discounts on coordinate 1, points on the boundaries."""
    kp = with_events(radial(D, R.K_NORMAL), 3, 1)
    vals = tuple(v for e in kp.events for v in e[:2])
    run_xgrad(gpm, kp, 256, 191, True, xgrad_family(D, True), "xgrad events D=%d" % D, boundary=(1, vals))


@pytest.mark.parametrize("name,npad,n", [("periodic", 256, 256), ("hyperpriors", 512, 449), ("max_terms", 256, 130),
                                         ("two5", 256, 1), ("two17", 256, 64)])
def test_xgrad_kinds_and_shapes(gpm, name, npad, n):
    kp = KPS[name]()
    if n == 1:   # one point: nothing to sum, gx[0] = 0 exactly
        X, alpha, K = operands("ld", npad, n, kp.ndim, seed=5)
        _, gx = gpm.xgrad_check(kp.hook(gpm), flat_x(X, n, npad, False)[:npad * kp.ndim], flat_alpha(alpha, n, npad),
                                xgrad_kinv(K, n, npad, npad), npad, n, npad, np.full(npad * kp.ndim, NAN64))
        assert np.all(bits(gx[:kp.ndim]) == 0) and same_bits(gx[kp.ndim:], np.full((npad - 1) * kp.ndim, NAN64))
        return
    run_xgrad(gpm, kp, npad, n, False, xgrad_family(kp.ndim, False), "xgrad %s n=%d/%d" % (name, n, npad))


def test_zz_report_ratios():
    """The largest |got - ref| / e_q per instance family seen in this run (always passes; -s shows it)."""
    for f in sorted(RATIOS):
        print("FAMILY %-14s max |got - ref| / e_q = %.3f" % (f, RATIOS[f]))
