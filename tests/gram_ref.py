"""Host references of the kernels that EVALUATE the similarity (gogp_amd/csrc/gram.hip: the Gram matrix, its 2-D
block-cyclic cut, the cross-covariance, the prior, the exact matrix-vector product of the fp32 path's residual) and of the
forecast derivatives (pgrad.hip: pgrad_kernel, pgrad_final_kernel), written from the formulas in kern_eval.h's header
(kernel/kernel.go:23-26, 44-47, 70-73, 89-92; tutorial/events/kernel/kernel.go:33-44), not from the device code:

    k(a, b) = d(a, b) sum_t c_t f_t(.)  (+ noise_var on the diagonal of the Gram matrix)
    radial kinds:  s = sum_d ((a_d - b_d) / l_d)^2, f = exp(-s / 2) | (1 + sqrt(3 s)) exp(-sqrt(3 s)) | (1 + sqrt(5 s) + q s)
                   exp(-sqrt(5 s)) with q = 1 (the reference's integer 5 / 3) or 5 / 3 (textbook)
    periodic:      s = sum_d (sin(w |a_d - b_d|) / l_d)^2, f = exp(-2 s)
    d(a, b):       the discount of the first event (list order) that separates the two points on coordinate ev_axis, 1 if none

The parameter block (KP), f and its derivatives (_radial), the discount, gamma_k, u and EPS_FN are those of
tests/grad_reduce_ref.py; the derivative dk/dz of the forecast derivatives is its `xgrad` pair terms, taken over the pairs
(test point, observation); the block-cyclic cut of one global matrix is the layout model of tests/shard_kernels_ref.py.

Every quantity comes as numpy.longdouble values (mode "ld") with a bound for an fp64 evaluation beside it, or (mode "f64") as
the plain float64 evaluation of the same formulas -- the run the bound is about (tests/test_gram_hooks_cpu.py).  u = 2^-53,
gamma_k = k u / (1 - k u).  EPS_FN = 4 u per transcendental call is the project's stated ASSUMPTION about the device math
library (tests/grad_reduce_ref.py: its accuracy table is not among this repository's documents); it is kept here.  The bounds
come from this model and the inputs only, never from a device run:

  one element   e_ij = d_ij sum_t |c_t| (|f_t'(s)| gamma_{D+2} s + calls_t EPS_FN |f_t|)      calls: 1 (exp), 2 (sqrt, exp)
                     + periodic terms: |c_t| f_t (EPS_FN + 2 ds), ds the error of the argument s: per dimension the sine's
                       EPS_FN and the 2 u of its argument w |a_d - b_d|, 3 u for the scaling and the square, gamma_D for the sum
                     + gamma_{nterms+2} (d_ij sum_t |c_t f_t| + noise_var on the diagonal)     the products, the sum over the
                       terms, the discount and the noise
                     + 2^-24 |k_ij| for a float output (one rounding)
  a matrix-vector row   gamma_n sum_j |K_ij v_j| + sum_j e_ij |v_j|    (+ u |r_i| for the residual's y_i - (K v)_i)
  dmu, dsigma   the same form over the observations (grad_reduce_ref's _Acc), the division by 2 sigma taken as one ulp (2 u)

The bound's own sums run in float64 on non-negative terms and are inflated by 1 + 2^-30."""
import numpy as np

import shard_kernels_ref as S
from cases import NAN32, NAN64  # noqa: F401  (the tests take the sentinels from here)
from grad_reduce_ref import (EPS_FN, K_MATERN32, K_MATERN52, K_MATERN52_TEXTBOOK, K_NORMAL, K_PERIODIC, KP, LD,  # noqa: F401
                             MAX_EVENTS, MAX_NDIM, MAX_TERMS, U, _Acc, _f64, _pair_terms, _radial, discount, gamma)

_INFLATE = 1.0 + 2.0 ** -30
F64, F32 = np.float64, np.float32


def pair_values(kp, A, B, mode="ld", diag_noise=False, out32=False):
    """k(a_i, b_j) for the rows of A (ma, D) against the rows of B (mb, D) -- with diag_noise the Gram matrix of A == B,
    noise_var on its diagonal -- and the bound e_ij of an fp64 evaluation (with out32: rounded once to float)."""
    assert mode in ("ld", "f64")
    dt = LD if mode == "ld" else F64
    D = kp.ndim
    Aa, Bb = np.asarray(A, F64)[:, :D].astype(dt), np.asarray(B, F64)[:, :D].astype(dt)
    shape = (len(Aa), len(Bb))
    k, e, mag = np.zeros(shape, dt), np.zeros(shape), np.zeros(shape)
    for T in kp.terms:
        c, ac, il, ilf, kind = dt(T["c"]), abs(T["c"]), T["inv_len"].astype(dt), T["inv_len"], T["kind"]
        s = np.zeros(shape, dt)
        if kind != K_PERIODIC:
            for d in range(D):
                s += ((Aa[:, None, d] - Bb[None, :, d]) * il[d]) ** 2
            f, f1, _ = _radial(kind, s, dt)
            e += ac * (_f64(f1) * gamma(D + 2) * _f64(s) + (1 if kind == K_NORMAL else 2) * EPS_FN * _f64(f))
        else:
            w, ds = dt(T["w"]), np.zeros(shape)
            for d in range(D):
                phi = w * np.abs(Aa[:, None, d] - Bb[None, :, d])
                sn, cs = np.sin(phi), np.cos(phi)
                dd2 = (sn * il[d]) ** 2
                s += dd2
                ds += 2 * _f64(sn) * ilf[d] ** 2 * (_f64(cs) * _f64(phi) * 2 * U + _f64(sn) * EPS_FN) + 3 * U * _f64(dd2)
            ds += gamma(D) * _f64(s)
            f = np.exp(-2 * s)
            e += ac * _f64(f) * (EPS_FN + 2 * ds)
        k += c * f
        mag += ac * _f64(f)
    if kp.events:
        disc = discount(kp.events, np.asarray(A, F64)[:, kp.ev_axis], np.asarray(B, F64)[:, kp.ev_axis])
        k, e, mag = k * disc.astype(dt), e * np.abs(disc), mag * np.abs(disc)
    if diag_noise:
        assert shape[0] == shape[1]
        i = np.arange(shape[0])
        k[i, i] += dt(kp.noise_var)
        mag[i, i] += abs(kp.noise_var)
    e += gamma(len(kp.terms) + 2) * mag
    if out32:
        e += 2.0 ** -24 * _f64(k)
    return k, e * _INFLATE


def padded_gram(kp, X, n, npad, mode="ld", out32=False):
    """The npad x npad Gram matrix as the launches leave it where they write: K (both triangles) on the leading n x n,
    identity beyond; and the bound (0 on the padding: those elements are exact)."""
    k, e = pair_values(kp, X[:n], X[:n], mode, True, out32)
    G, E = np.eye(npad, dtype=k.dtype), np.zeros((npad, npad))
    G[:n, :n], E[:n, :n] = k, e
    return G, E


def padded_cross(kp, X, n, npad, Z, m, mpad, mode="ld", out32=False):
    """KsT (mpad x npad): [j][i] = k(x_i, z_j), zero for i >= n or j >= m; and the bound."""
    k, e = pair_values(kp, Z[:m], X[:n], mode, False, out32)
    G, E = np.zeros((mpad, npad), k.dtype), np.zeros((mpad, npad))
    G[:m, :n], E[:m, :n] = k, e
    return G, E


def split_written(npad):
    """Elements launch_gram_lower_split writes: the 64 x 64 tiles on and below the diagonal, whole."""
    t = np.arange(npad) // 64
    return t[:, None] >= t[None, :]


def local_cut(G, nb, Pr, Pc, pr, pc):
    """What launch_gram_local leaves on rank (pr, pc) of the Pr x Pc grid, from the padded global matrix G: (local values,
    written, zeroed) -- the rank's local rows and columns of G; `zeroed`: distribution blocks strictly above the diagonal
    (exact zeros); neither written nor zeroed: the 64-tiles above the diagonal inside a diagonal block (nb >= 128)."""
    NB = G.shape[0] // nb
    gr, gc = S.global_rows(NB, nb, Pr, pr), S.global_rows(NB, nb, Pc, pc)
    loc = G[np.ix_(gr, gc)]
    I, J = (gr // nb)[:, None], (gc // nb)[None, :]
    ti, tj = (gr // 64)[:, None], (gc // 64)[None, :]
    zeroed = I < J
    written = ~zeroed & (ti >= tj)
    return loc, written, zeroed


def prior_values(kp):
    """k(z, z): the sum of the output scales, exactly (s = 0: f = 1 for every kind; no discount between equal points)."""
    return sum(T["c"] for T in kp.terms)


def share_tiles(npad, part_idx, nparts):
    """Column tiles [t0, t1) of share part_idx of nparts of the matrix-vector product: ceil(ntile / nparts) each, the last
    ones short or empty."""
    ntile = npad // 64
    per = -(-ntile // nparts)
    return min(ntile, part_idx * per), min(ntile, (part_idx + 1) * per)


def matvec(kp, X, n, v, y=None, cols=None, mode="ld"):
    """(K v)_i over the columns `cols` (default all below n) for i < n, or y - K v; and its bound."""
    dt = LD if mode == "ld" else F64
    cols = np.arange(n) if cols is None else np.asarray(cols)
    cols = cols[cols < n]
    k, e = pair_values(kp, X[:n], X[:n], mode, True)
    k, e, vv = k[:, cols], e[:, cols], np.asarray(v, F64)[cols]
    val = k @ vv.astype(dt)
    bnd = gamma(max(n, 1)) * (_f64(k) @ np.abs(vv)) + e @ np.abs(vv)
    if y is not None:
        val = np.asarray(y, F64)[:n].astype(dt) - val
        bnd = bnd + U * _f64(val)
    return val, bnd * _INFLATE


def pgrad_sums(kp, X, n, Z, m, alpha, Wt, sigma, mode="ld"):
    """dmu[j][d] = sum_i alpha_i dk(z_j, x_i)/dz_jd and dsigma[j][d] = -2 sum_i Wt[j][i] dk(z_j, x_i)/dz_jd / (2 sigma_j),
    each (m, D), with their bounds: (dmu, e_dmu, dsigma, e_dsigma).  sigma_j <= 0 gives what the division yields."""
    dt = LD if mode == "ld" else F64
    D = kp.ndim
    P = np.concatenate([np.asarray(Z, F64)[:m, :D], np.asarray(X, F64)[:n, :D]])  # the test points, then the observations
    rows, cols = np.arange(m), m + np.arange(n)
    disc = discount(kp.events, P[rows, kp.ev_axis], P[cols, kp.ev_axis]).astype(dt)
    Ws = [np.broadcast_to(np.asarray(alpha, F64)[:n].astype(dt), (m, n)) * disc, np.asarray(Wt, F64)[:m, :n].astype(dt) * disc]
    acc = _Acc(Ws, dt, (m, D), n * len(kp.terms), m + n)
    _pair_terms(kp, P, m + n, acc, "diff", dt, True, rows, cols)
    sg = np.asarray(sigma, F64)[:m].astype(dt)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        dsig = (-2 * acc.val[1]) / (2 * sg)
        e_dsig = acc.bnd[1] / _f64(sg) + 2 * U * _f64(dsig)
    return acc.val[0], acc.bnd[0], dsig, e_dsig * _INFLATE


def pgrad_slabs(npad, m):
    """launch_pgrad's split of the npad / 64 row tiles for m test points, restated: at most 1024 / ceil(m / 4) slabs (one at
    least, no more than tiles), evened out so that no slab is empty.  Returns (slabs, tiles per slab)."""
    tiles, mblk = npad // 64, -(-m // 4)
    nslab = min(tiles, max(1, 1024 // mblk))
    tps = -(-tiles // nslab)
    return -(-tiles // tps), tps


# ---- the cases the GPU test (tests/test_gram_kernels.py) walks and the CPU test (tests/test_gram_hooks_cpu.py) judges the
# float64 evaluation on -----------------------------------------------------------------------------------------------
import functools  # noqa: E402

#: the staging loops are ragged below D = 4; 62 .. 64 are the sizes around the 64 KB of dynamic LDS
LD_DIMS = [1, 2, 3, 5, 8, 17, 33, 62, 63, 64]
RADIAL = {"normal": K_NORMAL, "matern32": K_MATERN32, "matern52": K_MATERN52, "matern52tb": K_MATERN52_TEXTBOOK}
LD_SHAPE = dict(npad=256, n=193, m=65, mpad=128)
#: events on a grid of eighths, where the coordinates of the event axis lie too: some are exactly a `from`, some a `to`
EVENT_SETS = {
    1: [(-0.5, 0.25, 0.7)],
    3: [(-1.0, -0.5, 0.9), (-0.25, 0.5, 0.6), (0.75, 1.5, 0.35)],
    MAX_EVENTS: [(-2.0 + e / 8.0, -2.0 + e / 8.0 + (0.0625 if e % 2 else 0.125) + (e % 3) / 8.0, 0.3 + 0.02 * e)
                 for e in range(MAX_EVENTS)],  # every other `to` lies between two grid points
    2: [(-0.625, 0.125, 0.8), (0.5, 1.0, 0.45)],
}


def terms_of(kind, D):
    """The terms of a named kernel at D dimensions: length scales ~ sqrt(D), so that s stays of order one."""
    il = 1.0 / (0.8 * np.sqrt(D))
    per = dict(kind=K_PERIODIC, c=0.9, w=np.pi / 0.45, inv_len=1.3 * il)
    if kind in RADIAL:
        return [dict(kind=RADIAL[kind], c=1.3, inv_len=il)]
    if kind == "periodic":
        return [per]
    if kind == "max_terms":
        return [dict(kind=K_NORMAL, c=0.7, inv_len=il), dict(kind=K_MATERN32, c=1.1, inv_len=0.6 * il),
                dict(kind=K_MATERN52_TEXTBOOK, c=0.4, inv_len=1.7 * il), dict(per, c=0.25)]
    if kind == "hyperpriors":  # c Matern52 + c' Periodic with a scaled period (tutorial/hyperpriors/kernel/kernel.go:23-24)
        return [dict(kind=K_MATERN52, c=1.0, inv_len=il / 0.5), dict(kind=K_PERIODIC, c=1.3, w=np.pi / (10.0 * 0.6), inv_len=il)]
    assert kind == "ard"
    return [dict(kind=K_NORMAL, c=1.2, ard=True, inv_len=il * (1.0 + np.arange(D) / (2.0 * D)))]


#: (kernel, D, number of events, event axis) of the long-double mode
LD_CASES = [(k, D, 0, 0) for D in LD_DIMS for k in list(RADIAL) + ["periodic"]]
LD_CASES += [("max_terms", D, 0, 0) for D in (1, 3, 17, 64)] + [("hyperpriors", 1, 0, 0), ("hyperpriors", 5, 0, 0)]
LD_CASES += [("ard", 5, 0, 0), ("ard", 64, 0, 0)]
LD_CASES += [("matern32", 1, 1, 0), ("normal", 3, 3, 2), ("max_terms", 3, 3, 1), ("matern52", 5, MAX_EVENTS, 3),
             ("periodic", 2, MAX_EVENTS, 1), ("normal", 62, 2, 61), ("hyperpriors", 62, 2, 5), ("normal", 64, 2, 3),
             ("max_terms", 64, 2, 63)]


def case_id(c):
    return "%s-D%d" % c[:2] + ("-ev%d@%d" % c[2:] if c[2] else "")


def kp_of(case, noise_var=0.37):
    kind, D, nev, axis = case
    return KP(D, terms_of(kind, D), EVENT_SETS[nev] if nev else (), axis, noise_var)


@functools.lru_cache(maxsize=None)
def problem(D, npad, n, m=1, mpad=64, ev_axis=-1, seed=0, integer=False):
    """Inputs of one launch: X (npad rows and the hooks' slack, payload NaNs from row n on), Z (mpad rows, NaNs from row m
    on), v and y (npad, NaNs / zeros from n on).  ev_axis >= 0: that coordinate lies on the grid of eighths in [-2, 2].
    integer: v and y small integers (the exact mode)."""
    rng = np.random.default_rng([71, D, npad, n, m, mpad, ev_axis + 1, seed, int(integer)])
    X, Z = np.full(npad * D + MAX_NDIM, NAN64), np.full(mpad * D, NAN64)
    x, z = rng.uniform(-1.0, 1.0, (n, D)), rng.uniform(-1.0, 1.0, (m, D))
    if ev_axis >= 0:
        x[:, ev_axis], z[:, ev_axis] = rng.integers(-16, 17, n) / 8.0, rng.integers(-16, 17, m) / 8.0
    X[:n * D], Z[:m * D] = x.reshape(-1), z.reshape(-1)
    v, y = np.full(npad, NAN64), np.full(npad, NAN64)
    if integer:
        v[:n], y[:n] = rng.integers(-8, 9, n), rng.integers(-8, 9, n)
    else:
        v[:n], y[:n] = rng.standard_normal(n), rng.standard_normal(n)
    return S._frozen(dict(X=X, Z=Z, x=x, z=z, v=v, y=y))


# exact mode: inv_len = 0, so s = 0 and f = 1 for every kind whatever the (finite) inputs; c a power of two, dyadic
# discounts, an integer noise: k_ij = d_ij sum_t c_t (+ noise) bit for bit in any evaluation order
EXACT_EVENTS = [(-0.5, 0.25, 0.5), (0.375, 1.0, 0.25), (-1.5, -1.0, 0.75)]
EXACT_KERNELS = {
    "radial1": [dict(kind=K_NORMAL, c=4.0, inv_len=0.0)],
    "generic": [dict(kind=K_MATERN32, c=2.0, inv_len=0.0), dict(kind=K_PERIODIC, c=0.5, w=np.pi / 0.45, inv_len=0.0)],
}


def exact_kp(which, D, ev=False, ev_axis=0, c_scale=1.0, noise_var=3.0):
    terms = [dict(T, c=T["c"] * c_scale) for T in EXACT_KERNELS[which]]
    return KP(D, terms, EXACT_EVENTS if ev else (), ev_axis if ev else 0, noise_var)


def exact_gram(kp, x, n, npad):
    """The padded Gram matrix of the exact mode, in float64 (asserted exact)."""
    csum = sum(T["c"] for T in kp.terms)
    d = discount(kp.events, x[:n, kp.ev_axis], x[:n, kp.ev_axis])
    G = np.eye(npad)
    G[:n, :n] = csum * d + kp.noise_var * np.eye(n)
    assert np.array_equal(G * 2.0 ** 20, np.rint(G * 2.0 ** 20)), "exact mode: dyadic values"
    return G


def slab_columns(npad, nslab, t0, t1, share):
    """Per slab, the column tiles [a, b) launch_residual (share False: t0 = 0, t1 = ntile) and launch_kmatvec_share give it."""
    tps = -(-(t1 - t0) // nslab)
    if share:
        tps = max(1, tps)
    return [(min(t1, t0 + s * tps), min(t1, t0 + (s + 1) * tps)) for s in range(nslab)]


SPLIT_SHAPES = [(64, 1, 64), (64, 64, 64), (128, 100, 256), (256, 193, 64), (256, 256, 256), (320, 257, 128), (512, 449, 256)]
SPLIT_BIG = (2048, 2000, 256)
LOCAL_GRIDS = [(1, 1), (2, 1), (1, 2), (2, 3)]
CROSS_N, CROSS_M = [1, 63, 64, 65, 300], [1, 64, 65, 130]
PRIOR_M = [1, 255, 256, 257]
PGRAD_D, PGRAD_M, PGRAD_SHAPES = [1, 4, 5, 8, 9, 16, 17, 33, 64], [1, 3, 4, 5, 33], [(64, 1), (256, 193), (512, 449)]
PGRAD_KINDS = list(RADIAL) + ["periodic", "max_terms"]
#: every D with every m, the shapes and kernels rotating so that each D and each m meets every shape
PGRAD_CASES = [(PGRAD_KINDS[(2 * i + j) % len(PGRAD_KINDS)], D, 0, 0, m) + PGRAD_SHAPES[(i + j) % 3]
               for i, D in enumerate(PGRAD_D) for j, m in enumerate(PGRAD_M)]
PGRAD_CASES += [("matern52", 3, 3, 2, 5, 256, 193), ("periodic", 9, 1, 8, 33, 512, 449), ("max_terms", 17, MAX_EVENTS, 16, 4, 256, 193)]


@functools.lru_cache(maxsize=None)
def pgrad_problem(D, npad, n, m, ld, ev_axis=-1):
    """problem() and the weights of the two sums: alpha (npad, NaNs from n on), Wt (m rows of ld, NaNs from column n on),
    sigma (m, positive)."""
    p = dict(problem(D, npad, n, m, -(-m // 64) * 64, ev_axis, seed=5))
    rng = np.random.default_rng([72, D, npad, n, m])
    alpha, Wt = np.full(npad, NAN64), np.full(m * ld, NAN64).reshape(m, ld)
    alpha[:n], Wt[:, :n] = rng.standard_normal(n), rng.standard_normal((m, n))
    p.update(alpha=alpha, Wt=Wt.reshape(-1), sigma=rng.uniform(0.5, 2.0, m))
    return S._frozen(p)
