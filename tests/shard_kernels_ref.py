"""Host references of the kernels of the sharded path (gogp_amd/csrc/dist2d.hip and the "helpers of the sharded
evaluation" of solve.hip) and of the rest of solve.hip (the LML scalars, the fp64 trace, the layout kernels around the
factor, the one-line vector kernels), the operands the tests feed them and the shapes both tests/test_shard_kernels.py and
tests/test_shard_hooks_cpu.py walk.  Plain numpy.

The layout model.  Written from the comments of dist2d.hip and common.h, not from the kernels' index expressions: the
padded matrix has NB x NB tiles of nb x nb; tile (I, J) lives on the rank at grid position (I mod Pr, J mod Pc) of the
Pr x Pc grid; a rank's local tile row bi is the bi-th of ITS global tile rows in increasing order (columns likewise); its
chunk buffer holds, for each of its tile columns in order, one chunk: its tile rows of that block column one under the other,
each tile nb x nb row-major -- [bj][bi][r][c].  tiles_of() lists a rank's global tile indices; everything else follows
from it.

Reductions.  Every one has ONE evaluation, generic in the number type: in long double it is the reference, in float64 the
run the CPU test holds to the same bound.  Bounds (tests/finish_kernels_ref.py states the model): u = 2^-53; a sum of k
terms in any order, each term one rounded (or fused) product, errs by at most gamma_{k+1} sum |terms|; log within LOG_ULPS =
2 units in the last place, sqrt within 1; everything inflated by 1 + 2^-30.  Exact operands: small integers (and dyadic
m / 2^20 for single products) whose sums stay far below 2^53 in any order -- bit for bit.
"""
import functools
import math

import numpy as np

from cases import NAN32, NAN64
from finish_kernels_ref import LOG_ULPS, SQRT_ULPS, ULP
from substitution_ref import U, gamma

LD, F64, F32 = np.longdouble, np.float64, np.float32
_INFLATE = 1.0 + 2.0 ** -30
TDOT_SLAB = 256  # rows of one slab of chunk_tdot's partial sums

# ---- the shapes ----------------------------------------------------------------------------------------------------------
#: (Pr, Pc) -> the ranks (pr, pc) walked
GRIDS = {(1, 1): [(0, 0)], (2, 1): [(0, 0), (1, 0)], (1, 2): [(0, 0), (0, 1)],
         (2, 3): [(r, c) for r in range(2) for c in range(3)], (3, 2): [(0, 0), (2, 1), (1, 0)]}
#: (nb_shift, Pr, Pc, mult): NB = lcm(Pr, Pc) * mult tiles; small tiles for the walk, one case at the product's nb = 512
LAYOUT_CASES = [(6, Pr, Pc, mult) for (Pr, Pc) in GRIDS for mult in (1, 2)] + [(7, 2, 3, 1), (9, 2, 1, 1)]
#: chunk_sumsq also on 17 tiles of 64 on one rank: sum_kernel over 1088 local rows, beyond its 1024 threads
SUMSQ_CASES = LAYOUT_CASES + [(6, 1, 1, 17)]
TDOT_ROWS = [1, 4, 5, 8, 9, 255, 256, 257, 513]
TDOT_NB = [64, 128, 512]
TRANSPOSE_SQ_N = [32, 64, 256, 512]
TRANSPOSE_RECT = [(32, 96), (96, 32), (512, 64)]
PACK_S = 64 * 256  # threads of one block row of pack_blocks' grid
PACK_HALF_BLK = [1, PACK_S - 1, 4 * PACK_S, 4 * PACK_S + 1, 7 * PACK_S + 5]
CONVERT_COLS, CONVERT_ROWS = [1, 255, 256, 257, 512], [1, 3]
ZERO_UPPER_NPAD = [256, 512, 768, 1024]
ZERO_BLOCK_COLS = [2, 510, 512, 514]
EXTRACT_N = [1, 255, 256, 257]
PACK_LOWER = [(1, 256), (255, 256), (256, 256), (257, 512)]
VECTOR_COUNTS = [1, 255, 256, 257]
FILL_WRAP, ADD_INPLACE_WRAP = 4096 * 256 + 1, 1024 * 256 + 1  # one past the capped grids
LML_N = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
LML_BATCHED_N = [65, 1025]
#: (1023 .. 2049: sum_kernel, one workgroup of 1024 threads, adds the n row results -- around its width and a second trip)
TRACE_N = [1, 255, 256, 257, 513, 1023, 1024, 1025, 2049]
REDUCE_N = [1, 1023, 1024, 1025, 2049]
SIGMA_M = [1, 255, 256, 257]
RESIDUAL_ROWS, RESIDUAL_NRECV = [1, 5, None], [0, 1, 3]  # None: nb + 3
BATCH_K = 3


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, shape).astype(F64)


def _f(a):
    return np.abs(np.asarray(a)).astype(F64)


def nan_of(dt):
    return NAN64 if np.dtype(dt) == np.float64 else NAN32


def up256(n):
    return -(-n // 256) * 256


def rounded(a, prec):
    """The operand as a kernel of that matrix precision sees it, in float64."""
    return a if prec == 64 else a.astype(F32).astype(F64)


# ---- the layout model ----------------------------------------------------------------------------------------------------
def num_tiles(Pr, Pc, mult):
    return Pr * Pc // math.gcd(Pr, Pc) * mult


def tiles_of(NB, P, p):
    """The global tile indices of grid position p of P, in local order."""
    return [t for t in range(NB) if t % P == p]


def global_rows(NB, nb, P, p):
    """The global row (column) index of every local row of grid position p, in local order."""
    return np.concatenate([np.arange(t * nb, (t + 1) * nb) for t in tiles_of(NB, P, p)])


def chunks_of(G, nb, Pr, Pc, pr, pc, dt, keep=lambda I, J: True):
    """A rank's chunk buffer [bj][bi][r][c] of the global matrix G: the tiles keep(I, J) selects, sentinels in the others."""
    NB = G.shape[0] // nb
    Is, Js = tiles_of(NB, Pr, pr), tiles_of(NB, Pc, pc)
    out = np.full((len(Js), len(Is), nb, nb), nan_of(dt), dt)
    for bj, J in enumerate(Js):
        for bi, I in enumerate(Is):
            if keep(I, J):
                out[bj, bi] = G[I * nb:(I + 1) * nb, J * nb:(J + 1) * nb]
    return out


def local_matrix(G, nb, Pr, Pc, pr, pc):
    """A rank's tiles of G as one (mloc nb) x (nloc nb) matrix: the local rows and columns of the global one."""
    NB = G.shape[0] // nb
    return G[np.ix_(global_rows(NB, nb, Pr, pr), global_rows(NB, nb, Pc, pc))]


def upper(I, J):
    return J >= I


def lower(I, J):
    return I >= J


@functools.lru_cache(maxsize=None)
def layout_problem(nb_shift, Pr, Pc, mult, exact):
    """One global matrix G (npad x npad) and vector z for every rank of the grid."""
    nb, NB = 1 << nb_shift, num_tiles(Pr, Pc, mult)
    npad = NB * nb
    rng = _rng(11, nb_shift, Pr, Pc, mult, exact)
    if exact:
        G, z = _ints(rng, (npad, npad), 2), _ints(rng, npad)
    else:
        G, z = rng.standard_normal((npad, npad)), rng.standard_normal(npad)
    return _frozen(dict(G=G, z=z, nb=nb, NB=NB, npad=npad))


def sumsq_ns(nb, npad):
    """n of chunk_sumsq: a multiple of nb, the middle of a tile, 1, the padded size."""
    return sorted(n for n in {nb, npad - nb // 2 - 1, 1, npad, nb + nb // 2} if n <= npad)


def chunk_alpha_eval(G, z, nb, Pr, Pc, pr, pc, dt):
    """(global rows this rank writes, their partial sums, sum |terms|, terms per row) of chunk_alpha."""
    NB = G.shape[0] // nb
    rows, vals, mags, ks = [], [], [], []
    for I in tiles_of(NB, Pr, pr):
        cols = [np.arange(J * nb, (J + 1) * nb) for J in tiles_of(NB, Pc, pc) if J >= I]
        cols = np.concatenate(cols) if cols else np.arange(0)
        t = G[I * nb:(I + 1) * nb][:, cols].astype(dt) * z[cols].astype(dt)
        rows.append(np.arange(I * nb, (I + 1) * nb))
        vals.append(t.sum(1))
        mags.append(_f(t).sum(1))
        ks.append(np.full(nb, len(cols)))
    return np.concatenate(rows), np.concatenate(vals), np.concatenate(mags), np.concatenate(ks)


def chunk_alpha_ref(G, z, nb, Pr, Pc, pr, pc):
    rows, want, mag, k = chunk_alpha_eval(G, z, nb, Pr, Pc, pr, pc, LD)
    return rows, want, gamma(k + 1) * mag * _INFLATE


def chunk_sumsq_eval(G, nb, Pr, Pc, pr, pc, n, dt):
    """(part per local row, out) of chunk_sumsq: rows with global index >= n give exactly 0."""
    NB = G.shape[0] // nb
    part, ks = [], []
    for I in tiles_of(NB, Pr, pr):
        cols = [np.arange(J * nb, (J + 1) * nb) for J in tiles_of(NB, Pc, pc) if J >= I]
        cols = np.concatenate(cols) if cols else np.arange(0)
        t = G[I * nb:(I + 1) * nb][:, cols].astype(dt) ** 2
        live = (np.arange(I * nb, (I + 1) * nb) < n)
        part.append(np.where(live, t.sum(1), dt(0)))
        ks.append(np.where(live, len(cols), 0))
    part = np.concatenate(part)
    return part, part.sum(), np.concatenate(ks)


def chunk_sumsq_ref(G, nb, Pr, Pc, pr, pc, n):
    part, out, k = chunk_sumsq_eval(G, nb, Pr, Pc, pr, pc, n, LD)
    e_part = gamma(k + 1) * _f(part)
    e_out = e_part.sum() + gamma(len(part)) * float(part.sum())
    return (part, np.array([out])), (e_part * _INFLATE, np.array([e_out * _INFLATE]))


# ---- chunk_tdot -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tdot_problem(rows, nb, exact):
    rng = _rng(12, rows, nb, exact)
    if exact:
        return _frozen(dict(C=_ints(rng, (rows, nb), 2), v=_ints(rng, rows)))
    return _frozen(dict(C=rng.standard_normal((rows, nb)), v=rng.standard_normal(rows)))


def tdot_eval(C, v, dt):
    """(part [slab][c], out [c]) of chunk_tdot + finish."""
    t = C.astype(dt) * v.astype(dt)[:, None]
    nslab = -(-len(v) // TDOT_SLAB)
    part = np.stack([t[s * TDOT_SLAB:(s + 1) * TDOT_SLAB].sum(0) for s in range(nslab)])
    return part, part.sum(0)


def tdot_ref(C, v):
    part, out = tdot_eval(C, v, LD)
    t = _f(C.astype(LD) * v.astype(LD)[:, None])
    nslab = part.shape[0]
    mag = np.stack([t[s * TDOT_SLAB:(s + 1) * TDOT_SLAB].sum(0) for s in range(nslab)])
    e_part = gamma(TDOT_SLAB + 1) * mag
    e_out = e_part.sum(0) + gamma(nslab) * mag.sum(0)
    return (part, out), (e_part * _INFLATE, e_out * _INFLATE)


# ---- residual_block -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def residual_problem(rows, nb, nrecv, exact):
    """Ks, U (rows x nb) and nrecv received blocks; exact: dyadic operands whose sums of five are exact in float64 and
    need a rounding on their way to float."""
    rng = _rng(13, rows, nb, nrecv, exact)
    if exact:  # Ks: 21 bits, a float; U and the partials: 31 bits -- the exact fp64 difference does not fit a float
        dy = lambda shape, b: rng.integers(-(2 ** b) + 1, 2 ** b, shape).astype(F64) / 2.0 ** b  # noqa: E731
        return _frozen(dict(Ks=dy((rows, nb), 20), U=dy((rows, nb), 30), recv=dy((max(nrecv, 1), rows, nb), 30)[:nrecv]))
    draw = rng.standard_normal
    return _frozen(dict(Ks=draw((rows, nb)), U=draw((rows, nb)), recv=draw((max(nrecv, 1), rows, nb))[:nrecv]))


def residual_eval(Ks, U, recv, dt):
    u = U.astype(dt)
    for k in range(recv.shape[0]):
        u = u + recv[k].astype(dt)
    return Ks.astype(dt) - u


def residual_ref(Ks, U, recv):
    want = residual_eval(Ks, U, recv, LD)
    mag = _f(Ks) + _f(U) + _f(recv).sum(0)
    return want, gamma(recv.shape[0] + 1) * mag * _INFLATE


# ---- lml_scalars ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lml_problem(n, exact, seed=0):
    rng = _rng(14, n, exact, seed)
    if exact:
        d = rng.choice([0.25, 0.5, 2.0, 4.0, 16.0], n)
        return _frozen(dict(d=d, z=_ints(rng, n), y=_ints(rng, n), a=_ints(rng, n)))
    y = rng.standard_normal(n)  # (alpha of y's sign: y'alpha does not cancel, so its bound stays under judge()'s cap)
    return _frozen(dict(d=rng.uniform(1.5, 4.0, n), z=rng.standard_normal(n), y=y, a=y * rng.uniform(0.5, 1.5, n)))


def lml_eval(d, z, y, a, dt):
    """The five scalars of lml_scalars_kernel; a None: slot 2 is exactly 0."""
    d, z = d.astype(dt), z.astype(dt)
    s2 = dt(0) if a is None else (y.astype(dt) * a.astype(dt)).sum()
    return np.array([(dt(2) * np.log(d)).sum(), (z * z).sum(), s2, d.min(), d.max()], dt)


def lml_ref(d, z, y, a):
    want = lml_eval(d, z, y, a, LD)
    n = len(d)
    t0 = _f(LD(2) * np.log(d.astype(LD)))
    e0 = LOG_ULPS * ULP * t0.sum() + gamma(n) * t0.sum()
    e1 = gamma(n + 1) * float((z * z).sum())
    e2 = 0.0 if a is None else gamma(n + 1) * float(np.abs(y * a).sum())
    return want, np.array([e0, e1, e2, 0.0, 0.0]) * _INFLATE


# ---- alpha_from_y, trace_from_y -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rowblock_problem(n, npad, exact, seed=0):
    """Y (n rows of npad columns), z and alpha: of row i only the columns from the start of its 256-block on count."""
    rng = _rng(15, n, npad, exact, seed)
    if exact:
        return _frozen(dict(Y=_ints(rng, (n, npad), 2), z=_ints(rng, npad), a=_ints(rng, n)))
    return _frozen(dict(Y=rng.standard_normal((n, npad)) / np.sqrt(npad), z=rng.standard_normal(npad),
                        a=rng.uniform(2.0, 3.0, n)))


def block_start(n):
    return (np.arange(n) // 256) * 256


def block_mask(n, npad):
    """Element (i, q) is read: q >= the first column of row i's 256-block."""
    return np.arange(npad)[None, :] >= block_start(n)[:, None]


def alpha_eval(Y, z, dt):
    n, npad = Y.shape
    t = np.where(block_mask(n, npad), Y.astype(dt) * z.astype(dt)[None, :], dt(0))
    return t.sum(1), _f(t).sum(1)


def alpha_ref(Y, z):
    want, mag = alpha_eval(Y, z, LD)
    k = Y.shape[1] - block_start(Y.shape[0])
    return want, gamma(k + 1) * mag * _INFLATE


def trace_eval(Y, a, dt):
    """(part_i = alpha_i^2 - sum_{q >= q0(i)} Y_iq^2, their sum) of trace_from_y."""
    n, npad = Y.shape
    s = np.where(block_mask(n, npad), Y.astype(dt) ** 2, dt(0)).sum(1)
    part = a.astype(dt) ** 2 - s
    return part, part.sum(), s


def trace_ref(Y, a):
    part, out, s = trace_eval(Y, a, LD)
    k = Y.shape[1] - block_start(Y.shape[0])
    e_part = gamma(k + 1) * _f(s) + U * _f(a) ** 2 + U * _f(part)
    e_out = e_part.sum() + gamma(len(part)) * _f(part).sum()
    return (part, np.array([out])), (e_part * _INFLATE, np.array([e_out * _INFLATE]))


# ---- sum, dot, sumsq_info, logdet_block, sigma -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vec_problem(n, exact, seed=0):
    rng = _rng(16, n, exact, seed)
    if exact:
        return _frozen(dict(a=_ints(rng, n), b=_ints(rng, n)))
    a = rng.standard_normal(n)  # (b of a's sign: the dot product does not cancel)
    return _frozen(dict(a=a, b=a * rng.uniform(0.5, 1.5, n)))


def dot_eval(a, b, dt):
    return np.array([(a.astype(dt) * b.astype(dt)).sum()])


def dot_ref(a, b):
    return dot_eval(a, b, LD), np.array([gamma(len(a) + 1) * float(np.abs(a * b).sum()) * _INFLATE])


def logdet_eval(d, live, acc0, dt):
    """acc0 + sum over the live rows of 2 log d_i."""
    t = (dt(2) * np.log(d.astype(dt)))[:live]
    return np.array([dt(acc0) + t.sum()])


def logdet_ref(d, live, acc0):
    want = logdet_eval(d, live, acc0, LD)
    t = _f((LD(2) * np.log(d.astype(LD)))[:live]).sum()
    e = LOG_ULPS * ULP * t + gamma(max(live, 1)) * t + U * (abs(acc0) + t)
    return want, np.array([e * _INFLATE])


@functools.lru_cache(maxsize=None)
def sigma_problem(m, exact):
    """prior and q with prior > q; exact: the difference is a perfect square."""
    rng = _rng(17, m, exact)
    if exact:
        q = _ints(rng, m)
        return _frozen(dict(prior=q + rng.integers(0, 12, m).astype(F64) ** 2, q=q))
    q = rng.uniform(0.0, 1.0, m)
    return _frozen(dict(prior=q + rng.uniform(0.1, 2.0, m), q=q))


def sigma_eval(prior, q, dt):
    return np.sqrt(prior.astype(dt) - (0 if q is None else q.astype(dt)))


def sigma_ref(prior, q):
    want = sigma_eval(prior, q, LD)
    return want, _f(want) * (U / 2 + SQRT_ULPS * ULP) * _INFLATE + 1e-320
