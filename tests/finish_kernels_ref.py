"""Host references of the small kernels that finish a leave-one-out, multi-output or sparse evaluation
(gogp_amd/csrc/loo.hip; multi.hip: multi_dots_kernel; sparse.hip: the element-wise, scalar and Produce kernels), the
operands the tests feed them and the shapes both tests/test_finish_kernels.py and tests/test_finish_hooks_cpu.py walk.
Plain numpy: every kernel has ONE evaluation, written operation by operation as the kernel writes it and generic in the
number type -- in long double it is the reference, in float64 it is the run the CPU test holds to the same bounds.

Exact operands.  Integers in [-8, 8] (matrices of the symmetric product in [-2, 2]), scales that are powers of two,
kappa in {1/4, 1, 4, 16}: every product, quotient and partial sum is a small dyadic number far below 2^53 in any order,
1 / kappa and its root are powers of two, and the tests of Produce choose prior so that prior - q + t is a perfect square.
An fp64 kernel must return those values bit for bit.

Bounds (full-mantissa operands).  u = 2^-53.  Every +, -, * as the kernel writes it is allowed one rounding, u |result|;
-ffp-contract=on may fuse a product into the sum that follows, which only removes one of the roundings counted, so the
bound holds with and without the fusion.  A sum of k terms in any order is allowed gamma_k sum |terms|, gamma_k =
k u / (1 - k u) (Higham, section 3.1), on top of the terms' own bounds; exact zeros among the terms add nothing.  The bounds
of operands are propagated to first order through absolute values and the whole is inflated by 1 + 2^-30, which covers the
second-order terms (they are 2^-52 of the first-order ones) and the bound's own float64 arithmetic.

log, sqrt and division on the device.  ASSUMPTION: no accuracy table of the device library or of HIP's math functions is
installed with the toolchain this suite was written against (its documentation tree was searched for one), and nobody has
measured them on gfx950 for this project, so the model is the fallback the project agreed on: log within LOG_ULPS = 2 units
in the last place of its result, sqrt and division within SQRT_ULPS = DIV_ULPS = 1.  One unit in the last place of x is at
most ULP |x| = 2^-52 |x|.  The GPU tests print the share of each bound that was used (RATIO lines; DESIGN.md records them).
sqrt(s (1 + d)) = sqrt(s) (1 + d / 2) to first order: a root halves the relative error that enters it.

The constant 1/2 log 2 pi of loo_stats_kernel is the double nearest to 0.9189385332046727418, in the reference too: the
reference is the kernel's operation, not the formula's.
"""
import functools

import numpy as np

from substitution_ref import NAN64, U, gamma

LD = np.longdouble
ULP = 2.0 ** -52
LOG_ULPS, SQRT_ULPS, DIV_ULPS = 2.0, 1.0, 1.0
_INFLATE = 1.0 + 2.0 ** -30
HALF_LOG_2PI = 0.9189385332046727418  # the literal of loo_stats_kernel

STATS_CASES = [(256, 1), (256, 255), (256, 256), (512, 257), (512, 300), (768, 300)]
SYMV_CASES = [(256, 1), (256, 63), (256, 64), (256, 65), (256, 200), (256, 256), (512, 300)]
SYMV_EXACT_ONLY = (1280, 1100)  # lower_tile over 210 tiles
RANK2_CASES = [(256, 200), (512, 300)]
DOTS_CASES = [(n, T) for n in (1, 255, 256, 257, 1000) for T in (1, 3, 128)]
MPS = [256, 512]
NTS = [1, 3, 128]
SCALARS_MP, SCALARS_M = 512, [1, 255, 256, 257, 300, 512]
SUMSQ_N, SUMSQ_T = [1, 255, 257, 70001], [1, 5, 128]
MDOTS_CASES = [(M, T) for M in (1, 257, 300) for T in (1, 5)]
PAD_CASES = [(1, 1, 16, 128), (100, 5, 16, 128), (128, 16, 16, 128), (200, 17, 32, 256)]  # rows, T, kp, rpad
PREDICT_CASES = [(m, nc) for m in (1, 3, 4, 5, 9) for nc in (1, 63, 64, 65, 300)]
PREDICT_LD = 320
S4_DYADIC, S4_PLAIN = 0.25, 1.0 / 3.0


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


def _f(a):
    """|a| as float64 (the bounds are float64 arrays)."""
    return np.abs(np.asarray(a)).astype(np.float64)


def up256(n):
    return -(-n // 256) * 256


def padded(a, shape, fill=NAN64):
    """`a` in the leading corner of an array of `shape` filled with sentinels (or `fill`), flat."""
    out = np.full(shape, fill)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out.reshape(-1)


def with_tail(a, tail=5):
    """The flat array followed by `tail` sentinels: what lies behind an array a launch must leave alone."""
    return np.concatenate([np.asarray(a, np.float64).reshape(-1), np.full(tail, NAN64)])


def lower_flat(K, npad, ld, diag_only=False):
    """K^-1 as the loo kernels may see it: npad rows of ld, sentinels everywhere except the elements j <= i < n (the diagonal
    elements i < n alone with diag_only)."""
    n = K.shape[0]
    out = np.full((npad, ld), NAN64)
    if diag_only:
        out[np.arange(n), np.arange(n)] = np.diag(K)
    else:
        il = np.tril_indices(n)
        out[il] = K[il]
    return out.reshape(-1)


# ---- loo_stats_kernel ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stats_problem(npad, n, exact):
    rng = _rng(1, npad, n, exact)
    if exact:
        kap, a, y = rng.choice([0.25, 1.0, 4.0, 16.0], n), _ints(rng, n), _ints(rng, n)
    else:
        kap, a, y = rng.uniform(0.5, 4.0, n), rng.standard_normal(n), rng.standard_normal(n)
    return _frozen(dict(kap=kap, a=a, y=y))


def stats_eval(kap, a, y, npad, dt):
    """(mu, sigma, logp, v, sc, part) of loo_stats_kernel in the number type dt; v, sc: npad long, zero from n on."""
    kap, a, y = kap.astype(dt), a.astype(dt), y.astype(dt)
    n, half, one = len(kap), dt(0.5), dt(1.0)
    v = a / kap
    lp = half * np.log(kap) - half * a * v - dt(HALF_LOG_2PI)
    sc = np.sqrt((one + a * v) / kap)
    vp, sp, lpp = np.zeros(npad, dt), np.zeros(npad, dt), np.zeros(npad, dt)
    vp[:n], sp[:n], lpp[:n] = v, sc, lp
    return y - v, np.sqrt(one / kap), lp, vp, sp, lpp.reshape(-1, 256).sum(1)


def stats_ref(kap, a, y, npad):
    """The long-double values and their bounds, in the order of stats_eval."""
    want = stats_eval(kap, a, y, npad, LD)
    mu, sigma, lp, v, sc, part = want
    n = len(kap)
    aa, v_, t1, t2 = _f(a), v[:n], LD(0.5) * np.log(kap.astype(LD)), LD(0.5) * a.astype(LD) * v[:n]
    w = a.astype(LD) * v_
    e_v = DIV_ULPS * ULP * _f(v_)
    e_mu = e_v + U * (_f(mu) + e_v)
    e_sigma = _f(sigma) * (DIV_ULPS * ULP / 2 + SQRT_ULPS * ULP)
    rel = (aa * e_v + U * _f(w) + U * _f(1 + w)) / _f(1 + w) + DIV_ULPS * ULP
    e_sc = _f(sc[:n]) * (rel / 2 + SQRT_ULPS * ULP)
    e_lp = LOG_ULPS * ULP * _f(t1) + 0.5 * aa * e_v + U * _f(t2) + U * _f(t1 - t2) + U * _f(lp)
    pad = lambda e: np.concatenate([e, np.zeros(npad - n)])  # noqa: E731
    e_part = (pad(e_lp).reshape(-1, 256).sum(1) + gamma(256) * pad(_f(lp)).reshape(-1, 256).sum(1))
    return want, tuple(e * _INFLATE for e in (e_mu, e_sigma, e_lp, pad(e_v), pad(e_sc), e_part))


# ---- loo_scale_symv_kernel + loo_u_final_kernel ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def symv_problem(npad, n, exact):
    """K^-1 (n x n, symmetric), and sc and v of npad doubles, zero from n on: the precondition of the launcher."""
    rng = _rng(2, npad, n, exact)
    K = _ints(rng, (n, n), 2) if exact else rng.standard_normal((n, n))
    K = np.tril(K) + np.tril(K, -1).T
    sc, v = np.zeros(npad), np.zeros(npad)
    sc[:n] = rng.choice([0.5, 1.0, 2.0, 4.0], n) if exact else rng.uniform(0.5, 2.0, n)
    v[:n] = _ints(rng, n) if exact else rng.standard_normal(n)
    return _frozen(dict(K=K, sc=sc, v=v))


def symv_eval(K, sc, v, npad, dt):
    """(B, u): B = K^-1 diag(sc) on npad x npad and u = K^-1 v, zero from row / column n on."""
    n = K.shape[0]
    B, u = np.zeros((npad, npad), dt), np.zeros(npad, dt)
    B[:n, :n] = K.astype(dt) * sc[:n].astype(dt)[None, :]
    u[:n] = K.astype(dt) @ v[:n].astype(dt)
    return B, u


def symv_ref(K, sc, v, npad):
    n = K.shape[0]
    B, u = symv_eval(K, sc, v, npad, LD)
    e_u = np.zeros(npad)
    e_u[:n] = gamma(n) * (np.abs(K) @ np.abs(v[:n]))
    return (B, u), (U * _f(B) * _INFLATE, e_u * _INFLATE)


def symv_slots(nt, column_slot_tj=False):
    """The (slot, row) pairs of upart the workgroups of loo_scale_symv_kernel write, one entry per store: the tile (ti, tj),
    tj <= ti, stores its row sums to (tj, 64 ti + k) and, off the diagonal, its column sums to (ti, 64 tj + k).
    column_slot_tj: the pattern of a kernel that sent the column sums to slot tj instead."""
    out = []
    for ti in range(nt):
        for tj in range(ti + 1):
            out += [(tj, 64 * ti + k) for k in range(64)]
            if ti != tj:
                out += [(tj if column_slot_tj else ti, 64 * tj + k) for k in range(64)]
    return out


# ---- loo_rank2_kernel ------------------------------------------------------------------------------------------------------
def lower_tiles(npad):
    t = np.arange(npad) // 64
    return t[:, None] >= t[None, :]


@functools.lru_cache(maxsize=None)
def rank2_problem(npad, n, exact):
    rng = _rng(3, npad, n, exact)
    draw = (lambda s: _ints(rng, s)) if exact else rng.standard_normal
    u, alpha = np.zeros(npad), draw(n)
    u[:n] = draw(n)
    return _frozen(dict(G=draw((npad, npad)), u=u, alpha=alpha))


def rank2_eval(G, u, alpha, dt):
    """G - u alpha^T - alpha u^T on the leading n x n (the caller keeps what the launch does not touch)."""
    n = len(alpha)
    u_, a_ = u[:n].astype(dt), alpha.astype(dt)
    return G[:n, :n].astype(dt) - (u_[:, None] * a_[None, :] + a_[:, None] * u_[None, :])


def rank2_ref(G, u, alpha):
    n = len(alpha)
    want = rank2_eval(G, u, alpha, LD)
    p1, p2 = np.abs(np.outer(u[:n], alpha)), np.abs(np.outer(alpha, u[:n]))
    s = _f(want - G[:n, :n])
    return want, U * (p1 + p2 + s + _f(want)) * _INFLATE


# ---- sums of products: multi_dots, sparse_sumsq, sparse_multi_sumsq, sparse_multi_dots --------------------------------------
def dots_eval(A, B, dt):
    """sum over the last axis of A * B."""
    return (A.astype(dt) * B.astype(dt)).sum(-1)


def dots_ref(A, B):
    k = A.shape[-1]
    return dots_eval(A, B, LD), gamma(k) * (np.abs(A) * np.abs(B)).sum(-1) * _INFLATE


@functools.lru_cache(maxsize=None)
def dots_problem(tag, rows, k, exact):
    """Two rows x k operands of a kernel that sums k products per row."""
    rng = _rng(4, tag, rows, k, exact)
    draw = (lambda s: _ints(rng, s)) if exact else rng.standard_normal
    return _frozen(dict(A=draw((rows, k)), B=draw((rows, k))))


# ---- the Mp x Mp element-wise kernels ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def square_problem(tag, Mp, exact):
    """Three Mp x Mp matrices and a vector."""
    rng = _rng(5, tag, Mp, exact)
    draw = (lambda s: _ints(rng, s)) if exact else rng.standard_normal
    return _frozen(dict(B=draw((Mp, Mp)), Binv=draw((Mp, Mp)), GG=draw((Mp, Mp)), g=draw(Mp)))


def finish_b_eval(Bacc, inv_s2, dt):
    """I + sym(Bacc) inv_s2 from the elements a >= b of Bacc."""
    L = np.tril(Bacc).astype(dt)
    return np.eye(len(Bacc), dtype=dt) + (L + np.tril(L, -1).T) * dt(inv_s2)


def finish_b_ref(Bacc, inv_s2):
    want = finish_b_eval(Bacc, inv_s2, LD)
    p = _f(want - np.eye(len(Bacc), dtype=LD))
    return want, U * (p + np.eye(len(Bacc)) * _f(want)) * _INFLATE


def weights_eval(B, Binv, g, s4, dt):
    e = np.eye(len(B), dtype=dt)
    gg = (g.astype(dt)[:, None] * g.astype(dt)[None, :]) * dt(s4)
    return e - Binv.astype(dt) - gg, dt(2.0) * e - B.astype(dt) - Binv.astype(dt) - gg


def weights_ref(B, Binv, g, s4):
    T, S = weights_eval(B, Binv, g, s4, LD)
    e = np.eye(len(B), dtype=LD)
    gg = _f((e - Binv) - T)
    e_gg = 2 * U * gg
    e_T = e_gg + U * _f(e - Binv) + U * _f(T)
    e_S = e_gg + U * _f(2 * e - B) + U * _f(2 * e - B - Binv) + U * _f(S)
    return (T, S), (e_T * _INFLATE, e_S * _INFLATE)


def multi_weights_eval(B, Binv, GG, nT, s4, dt):
    e = np.eye(len(B), dtype=dt)
    gg = GG.astype(dt) * dt(s4)
    return dt(nT) * (e - Binv.astype(dt)) - gg, dt(nT) * (dt(2.0) * e - B.astype(dt) - Binv.astype(dt)) - gg


def multi_weights_ref(B, Binv, GG, nT, s4):
    Tm, S = multi_weights_eval(B, Binv, GG, nT, s4, LD)
    e = np.eye(len(B), dtype=LD)
    gg, d, d1, d2 = _f(GG.astype(LD) * LD(s4)), _f(e - Binv), _f(2 * e - B), _f(2 * e - B - Binv)
    e_T = U * (nT * d + nT * d + gg + _f(Tm))
    e_S = U * (nT * (d1 + d2) + nT * d2 + gg + _f(S))
    return (Tm, S), (e_T * _INFLATE, e_S * _INFLATE)


# ---- sparse_scalars_kernel -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalars_problem(M, exact):
    """The diagonals of C, B, Binv and the vectors r, g (M long).  Every term of every sum is positive, as in the product
    (C_ii > 1 here; B = I + V V^T / s2 has B_ii >= 1, Binv_ii > 0 and r^T g = r^T B^-1 r > 0): no sum cancels."""
    rng = _rng(6, M, exact)
    if exact:
        c, b, bi = rng.integers(2, 9, M) * 1.0, rng.integers(1, 9, M) * 1.0, rng.integers(1, 9, M) * 1.0
        r = rng.integers(1, 9, M) * 1.0
        g = r * rng.choice([0.5, 1.0, 2.0], M)
    else:
        c, b, bi = rng.uniform(1.5, 4.0, M), rng.uniform(1.0, 3.0, M), rng.uniform(0.1, 1.0, M)
        r = rng.standard_normal(M)
        g = r * rng.uniform(0.2, 1.0, M)
    return _frozen(dict(c=c, b=b, bi=bi, r=r, g=g))


def scalars_eval(c, b, bi, r, g, dt):
    c, b, bi, r, g = (x.astype(dt) for x in (c, b, bi, r, g))
    return np.array([(dt(2.0) * np.log(c)).sum(), (b - dt(1.0)).sum(), bi.sum(), (r * g).sum(), (g * g).sum()], dtype=dt)


def scalars_ref(c, b, bi, r, g):
    want = scalars_eval(c, b, bi, r, g, LD)
    M = len(c)
    terms = [_f(2 * np.log(c.astype(LD))), _f(b - 1.0), _f(bi), _f(r * g), _f(g * g)]
    own = [LOG_ULPS * ULP * terms[0], U * terms[1], 0.0 * terms[2], U * terms[3], U * terms[4]]
    e = np.array([np.sum(o) + gamma(M) * np.sum(t) for o, t in zip(own, terms)])
    return want, e * _INFLATE


# ---- sparse_predict_kernel / sparse_multi_sigma_kernel -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def predict_problem(m, ncols, exact):
    rng = _rng(7, m, ncols, exact)
    if exact:
        A, V = _ints(rng, (m, ncols), 2), _ints(rng, (m, ncols), 2)
        q, dot = rng.integers(0, 9, m) * 1.0, _ints(rng, m)
        prior = rng.integers(1, 13, m) ** 2.0 + q - (A * V).sum(1)  # prior - q + t is a perfect square
        inv_s2 = 0.25
    else:
        A, V = rng.standard_normal((m, ncols)), rng.standard_normal((m, ncols))
        q, dot = rng.uniform(0.0, 1.0, m), rng.standard_normal(m)
        prior = q + 100.0 + rng.uniform(0.0, 50.0, m)  # prior - q + t stays far above zero: the kernels do not clamp
        inv_s2 = 1.0 / 3.0
    return _frozen(dict(A=A, V=V, prior=prior, q=q, dot=dot, inv_s2=inv_s2))


def predict_eval(A, V, prior, q, dot, inv_s2, dt):
    t = (A.astype(dt) * V.astype(dt)).sum(1)
    return dot.astype(dt) * dt(inv_s2), np.sqrt(prior.astype(dt) - q.astype(dt) + t)


def predict_ref(A, V, prior, q, dot, inv_s2):
    mu, sigma = predict_eval(A, V, prior, q, dot, inv_s2, LD)
    e_t = gamma(A.shape[1]) * (np.abs(A) * np.abs(V)).sum(1)
    s = sigma * sigma
    assert (s >= 1.0).all()
    e_s = e_t + U * _f(prior - q) + U * _f(s)
    e_sigma = e_s / (2 * _f(sigma)) + SQRT_ULPS * ULP * _f(sigma)
    return (mu, sigma), (U * _f(mu) * _INFLATE, e_sigma * _INFLATE)
