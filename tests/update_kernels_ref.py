"""Host references of the kernels behind Append, Remove, ProduceGradient's skinny product and ProduceCovariance
(gogp_amd/csrc/append.hip, remove.hip, pgrad.hip: bwd_panel_kernel, pcov.hip), and the operands the tests feed them.
Plain numpy in integers and long double, in the style of substitution_ref.py, whose layouts and gamma are reused.

Exact operands.  Matrices in {-1, 0, 1}, vectors in [-8, 8], dyadic similarity parameters: every partial sum is an integer
(or a small dyadic) far below 2^53 in any order, so an fp64 kernel must return the reference bit for bit.  The similarity
is kept exact by inv_len = 0 and kind NORMAL: every scaled difference is (x - x') * 0 = 0, exp(-0.0) == 1, and
simil_value returns c whatever the points; with events the pair's value is c or c * disc (kern_eval.h: a pair is
discounted by the first event whose from / to mask bit differs between the two points).

Full-mantissa operands.  A product of K terms summed in any order errs by at most gamma_K sum |terms| (Higham, section
3.1; FMA and MFMA chains only tighten it).  remove_block's recurrence gets a RUNNING bound: every sqrt, division and fma
adds u |result| and the operands' bounds are propagated through absolute values (products of two bounds included); the
bound's own float64 arithmetic is inflated by 1 + 2^-30.
"""
import functools

import numpy as np

from substitution_ref import (NAN64, TS_SOL_COMPACT, TS_SOL_GRANULE, TS_SOL_PAIRED, U, encode_compact, encode_granule,
                              encode_paired, gamma)

TS_SOL_ROWS = 3
P = 256
RB = 128  # columns per step of remove_block_kernel
APPEND_PART = 64 * 64 + 64
_INFLATE = 1.0 + 2.0 ** -30
LD = np.longdouble


def _frozen(*arrs):
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrs


# ---- the similarity, kept exact ------------------------------------------------------------------------------------------
C_EXACT, NOISE_EXACT = 4.0, 1.0
EVENTS = ((0.5, 0.75, 0.5), (2.0, 3.0, 0.25))  # (from, to, discount): dyadic
EV_COORDS = (0.0, 0.5, 0.625, 0.75, 1.0, 2.5, 4.0)  # on both sides of every boundary, and ON two of them


def event_mask(x, events=EVENTS):
    m = 0
    for e, (frm, to, _) in enumerate(events):
        m |= int(frm <= x) << (2 * e)
        m |= int(to <= x) << (2 * e + 1)
    return m


def simil_exact(coords, ev, c=C_EXACT, events=EVENTS):
    """k(z_i, z_j) for inv_len = 0: c, times the discount of the first event between the two points' event coordinates."""
    m = len(coords)
    Kz = np.full((m, m), c)
    if ev:
        masks = [event_mask(x, events) for x in coords]
        for i in range(m):
            for j in range(m):
                d = masks[i] ^ masks[j]
                if d:
                    Kz[i, j] = c * events[((d & -d).bit_length() - 1) >> 1][2]
    return Kz


def points(m, seed, ev_axis=1, ndim=2):
    """m points: the event coordinate from EV_COORDS, the others arbitrary (inv_len = 0 makes them irrelevant)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, ndim))
    X[:, ev_axis] = rng.choice(EV_COORDS, m)
    if m >= 2:
        X[0, ev_axis], X[m - 1, ev_axis] = 0.0, 4.0  # some pair is discounted
    return X


# ---- append_gram -----------------------------------------------------------------------------------------------------------
def solution_layout(j0, cnt):
    """(kind, width) trsm_small_solution names for the fp64 launch of the right-hand sides j0 .. j0 + cnt - 1."""
    if j0 == 0 and cnt == 1:
        return TS_SOL_GRANULE, 1
    for w in (1, 2, 4, 8):
        if cnt <= w:
            return TS_SOL_COMPACT, w
    return (TS_SOL_PAIRED, 16) if cnt <= 16 else (TS_SOL_PAIRED, 32)


def encode_source(V, kind, width, off, ldrows=None):
    """Raw bytes of a source of append_gram: `off` bytes of sentinel, then V (npc x cols) in the layout, the columns
    cols .. width - 1 of a wider layout (and, ROWS, the columns from npc on of every row) sentinels."""
    npc, cols = V.shape
    if kind == TS_SOL_ROWS:
        full = np.full((cols, width), NAN64)
        full[:, :npc] = V.T
        body = full.reshape(-1).view(np.uint8)
    elif kind == TS_SOL_GRANULE:
        assert cols == 1 and width == 1
        body = encode_granule(V[:, 0])
    else:
        full = np.full((npc, width), NAN64)
        full[:, :cols] = V
        body = (encode_paired if kind == TS_SOL_PAIRED else encode_compact)(full, width)
    assert off % 16 == 0
    head = np.full(off // 8, NAN64).view(np.uint8)
    return np.ascontiguousarray(np.concatenate([head, body, head]))


def gram_sources(V, rows_layout=False):
    """((raw, kind, width, off) x 2, m0) as gogp_append hands V to launch_append_gram: the columns (0, min(m, 32)) and
    (32, m - 32) in the layouts of their launches; rows_layout: the fallback's single TS_SOL_ROWS source."""
    npc, m = V.shape
    if rows_layout:
        s = (encode_source(V, TS_SOL_ROWS, npc + 6, 48), TS_SOL_ROWS, npc + 6, 48)
        return s, s, m
    m0 = min(m, 32)
    k0, w0 = solution_layout(0, m0)
    s0 = (encode_source(V[:, :m0], k0, w0, 272), k0, w0, 272)
    if m <= 32:
        return s0, s0, m0
    k1, w1 = solution_layout(32, m - 32)
    return s0, (encode_source(V[:, m0:], k1, w1, 32), k1, w1, 32), m0


def gram_written(m):
    """Mask (64 x 64) of the entries of a part's Gram slot that append_gram writes: the 16-tiles (w, tj <= w), w < ceil(m / 16)."""
    t = np.arange(64) // 16
    return (t[None, :] <= t[:, None]) & (t[:, None] < -(-m // 16))


def gram_ref(V, z, n, exact):
    """(G, dots, LT, eG, ed): per slab of 256 rows G = V_s^T V_s (64 x 64, zero-padded) and V_s^T z_s (64), LT = V[:n].T;
    eG, ed: the bounds of an fp64 evaluation (None when exact)."""
    npc, m = V.shape
    ns = npc // P
    it = np.int64 if exact else LD
    G, dots = np.zeros((ns, 64, 64), it), np.zeros((ns, 64), it)
    eG, ed = np.zeros((ns, 64, 64)), np.zeros((ns, 64))
    for s in range(ns):
        Vs, zs = V[s * P:(s + 1) * P].astype(it), z[s * P:(s + 1) * P].astype(it)
        G[s, :m, :m] = Vs.T @ Vs
        dots[s, :m] = Vs.T @ zs
        Va = np.abs(V[s * P:(s + 1) * P])
        eG[s, :m, :m] = gamma(P) * (Va.T @ Va) * _INFLATE
        ed[s, :m] = gamma(P) * (Va.T @ np.abs(z[s * P:(s + 1) * P])) * _INFLATE
    return (G, dots, V[:n].T.copy(), None, None) if exact else (G, dots, V[:n].T.copy(), eG, ed)


@functools.lru_cache(maxsize=None)
def gram_problem(npc, exact):
    """(V (npc x 64), z) shared by every m (the first m columns are used)."""
    rng = np.random.default_rng(8100 + npc + exact)
    if exact:
        return _frozen(rng.integers(-1, 2, (npc, 64)).astype(np.float64), rng.integers(-8, 9, npc).astype(np.float64))
    return _frozen(rng.standard_normal((npc, 64)), rng.standard_normal(npc))


# ---- append_commit ---------------------------------------------------------------------------------------------------------
def commit_problem(m, nslab, ev, seed, bad=None):
    """An append_commit whose every operation is exact.  L0: integer lower triangle, diagonal in 1 .. 3; z0 integers.  The
    parts sum to G = C - L0 L0^T (C = simil_exact + NOISE_EXACT I) and to y2 - L0 z0, split over nslab integer parts; what
    the kernel must not read of a part (above the diagonal, rows / entries from m on) holds sentinels.
    bad = (pivot, how): S is changed at [pivot][pivot] alone so that the pivot the factorisation meets there is 0 ("zero"),
    -3 ("neg") or NaN ("nan"); the pivots before it stay positive.
    Returns dict(X2, y2, part, L0, z0)."""
    rng = np.random.default_rng(seed)
    X2 = points(m, seed + 1)
    L0 = np.tril(rng.integers(-2, 3, (m, m)), -1).astype(np.float64) + np.diag(rng.integers(1, 4, m).astype(np.float64))
    z0 = rng.integers(-8, 9, m).astype(np.float64)
    C = simil_exact(X2[:, 1], ev) + NOISE_EXACT * np.eye(m)
    G = C - L0 @ L0.T  # dyadic (quarters at most), |.| < 2^10
    if bad is not None:
        p, how = bad
        G[p, p] += L0[p, p] ** 2 + {"zero": 0.0, "neg": 3.0, "nan": np.nan}[how]
    dots_total = rng.integers(-8, 9, m).astype(np.float64)
    y2 = L0 @ z0 + dots_total
    part = np.full((nslab, APPEND_PART), NAN64)
    low = np.tril(np.ones((m, m), bool))
    Gs = [rng.integers(-8, 9, (m, m)).astype(np.float64) for _ in range(nslab - 1)]
    ds = [rng.integers(-8, 9, m).astype(np.float64) for _ in range(nslab - 1)]
    Gs.append(G - sum(Gs))
    ds.append(dots_total - sum(ds))
    for q in range(nslab):
        slot = part[q, :4096].reshape(64, 64)
        slot[:m, :m][low] = Gs[q][low]
        part[q, 4096:4096 + m] = ds[q]
    return dict(X2=X2, y2=y2, part=part.reshape(-1), L0=L0, z0=z0)


# ---- bwd_panel -------------------------------------------------------------------------------------------------------------
def panel_rows(rows16):
    """Rows of A and C a launch works on: 16 rows16 up to 32, whole groups of 64 beyond."""
    return 16 * rows16 if rows16 <= 2 else -(-rows16 // 4) * 64


def panel_ref(A, B, C0, sub, exact):
    """(want, e): A B or C0 - A B.  e: gamma_K |A| |B|, and for sub the subtraction's own rounding on top."""
    K = A.shape[1]
    if exact:
        prod = A.astype(np.int64) @ B.astype(np.int64)
        assert (np.abs(A) @ np.abs(B)).max() + np.abs(C0).max() < 2.0 ** 53
        return (C0.astype(np.int64) - prod if sub else prod), None
    prod = A.astype(LD) @ B.astype(LD)
    e = gamma(K) * (np.abs(A) @ np.abs(B)) * _INFLATE
    if not sub:
        return prod, e
    want = C0.astype(LD) - prod
    return want, (e * (1 + U) + U * np.abs(want).astype(np.float64)) * _INFLATE


# ---- pcov ------------------------------------------------------------------------------------------------------------------
def slabs_ref(npad, m, ncu, wg_per_cu=4):
    """pcov_slabs restated: (slabs, columns per slab)."""
    tiles = -(-m // 64)
    pairs = tiles * (tiles + 1) // 2
    panels = max(1, npad // P)
    nslab = min(panels, max(1, -(-wg_per_cu * ncu // pairs)))
    pps = -(-panels // nslab)
    return -(-panels // pps), pps * P


def pair_list(m):
    t = -(-m // 64)
    return [(ti, tj) for ti in range(t) for tj in range(ti + 1)]


def pcov_ref(Vt, Kz, diag_add, nslab, cps, mo, exact):
    """(part, out, e_part, e_out).  part[slab][pair] = Vt[ti rows, slab columns] Vt[tj rows, slab columns]^T with the rows
    from m on masked; out = Kz - sum of the slabs (+ diag_add on the diagonal) on the leading m x m, identity up to mo.
    Vt None: no parts (the prior Gram matrix)."""
    m = Kz.shape[0]
    out = np.eye(mo).astype(np.float64 if exact else LD)
    if Vt is None:
        out[:m, :m] = Kz + diag_add * np.eye(m)
        return None, out, None, np.zeros((mo, mo))
    npad = Vt.shape[1]
    it = np.int64 if exact else LD
    pairs = pair_list(m)
    Vp = np.zeros((64 * -(-m // 64), npad), it)
    Vp[:m] = Vt
    Va = np.abs(Vp).astype(np.float64)
    part = np.zeros((nslab, len(pairs), 64, 64), it)
    e_part = np.zeros(part.shape)
    for s in range(nslab):
        c = slice(s * cps, min((s + 1) * cps, npad))
        for p, (ti, tj) in enumerate(pairs):
            part[s, p] = Vp[ti * 64:(ti + 1) * 64, c] @ Vp[tj * 64:(tj + 1) * 64, c].T
            e_part[s, p] = gamma(cps) * (Va[ti * 64:(ti + 1) * 64, c] @ Va[tj * 64:(tj + 1) * 64, c].T) * _INFLATE
    total = (Vp[:m] @ Vp[:m].T)
    if exact:
        assert (Va @ Va.T).max() + abs(diag_add) + np.abs(Kz).max() < 2.0 ** 40
        out[:m, :m] = Kz - total.astype(np.float64) + diag_add * np.eye(m)
        return part, out, None, None
    out[:m, :m] = Kz.astype(LD) - total + diag_add * np.eye(m)
    # one sum of npad products, nslab partial sums and three more terms, nested at most cps + nslab + 3 deep
    e_out = np.zeros((mo, mo))
    e_out[:m, :m] = gamma(cps + nslab + 3) * (np.abs(Kz) + abs(diag_add) + (Va @ Va.T)[:m, :m]) * _INFLATE
    return part, out, e_part, e_out


# ---- remove ----------------------------------------------------------------------------------------------------------------
def gather_ref(src, map_, n1, npad1, dst0):
    """launch_remove_gather on dst0 (npad1 x npad1): row i up to the end of its diagonal 256-block."""
    dst = dst0.copy()
    for i in range(npad1):
        ce = (i | (P - 1)) + 1
        if i < n1:
            dst[i, :ce] = 0.0
            dst[i, :i + 1] = src[map_[i], map_[:i + 1]]
        else:
            dst[i, :ce] = 0.0
            dst[i, i] = 1.0
    return dst


def w_ref(src, map_, rem, mc, mw, r0, n1, npad1, W0):
    """launch_remove_w on W0 (mw x npad1): rows r0 .. npad1 - 1 of every column."""
    W = W0.copy()
    W[:, r0:] = 0.0
    for j in range(mc):
        for i in range(r0, n1):
            if rem[j] < map_[i]:
                W[j, i] = src[map_[i], rem[j]]
    return W


def remove_operands(n1, cols, npad1=512, seed=0, zero_top=0, full=False):
    """(Lt (npad1 x npad1), W (cols x npad1)) of a removal as gather and remove_w leave them: the factor of a well
    conditioned Gram matrix of n1 + cols points whose scattered rows `rem` leave; W[j] is zero above its column's first
    affected row, and above row zero_top in every column (removals from behind zero_top only).  full: (Lt, W, L, rem)."""
    rng = np.random.default_rng(9000 + 13 * n1 + cols + seed)
    n0 = n1 + cols
    x = np.sort(rng.uniform(0, 0.02 * n0, n0))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 0.7) ** 2) + 0.5 * np.eye(n0)
    L = np.linalg.cholesky(K)
    lo = min(zero_top + cols, n0 - cols)
    rem = np.sort(rng.choice(np.arange(lo, n0), cols, replace=False)) if lo < n0 else np.arange(n0 - cols, n0)
    keep = np.ones(n0, bool)
    keep[rem] = False
    kept = np.flatnonzero(keep)
    Lt = np.eye(npad1)
    Lt[:n1, :n1] = np.tril(L[np.ix_(kept, kept)])
    W = np.zeros((cols, npad1))
    W[:, :n1] = np.where(kept[None, :] > rem[:, None], L[np.ix_(kept, rem)].T, 0.0)
    return (Lt, W, L, rem) if full else (Lt, W)


def remove_blocks_ref(L, W, kb0, kb1, n1, mode="ld", beta=None):
    """launch_remove_block for kb = kb0, kb0 + 128, .. kb1 on L (ld x ld, rows < n1 live) and W (mw x ld): the recurrence
    of remove_ref.remove_update.  mode "ld": long doubles; "f64": the plain float64 run.  Returns (L, W, beta) as the
    launches leave them in memory: the rows of W inside a block stay as the block found them (they are consumed in
    registers), the rows below are updated.  beta: see remove_residual (carried in from an earlier pass, or None)."""
    it = LD if mode == "ld" else np.float64
    L, W = L.astype(it), W.astype(it)
    mw = W.shape[0]
    beta = np.zeros(W.shape[1]) if beta is None else beta.copy()
    rho = 1.5 * gamma(mw + 8)
    cstep = 1.01 * (10 * rho + 2 * np.sqrt(2.0) * gamma(mw) + 3 * U)
    f = lambda a: np.abs(a).astype(np.float64)  # noqa: E731
    for kb in range(kb0, kb1 + 1, RB):
        ke = min(kb + RB, n1)
        Wk = W[:, kb:ke].copy()  # what stays in memory: the block's rows as the block found them
        for k in range(kb, ke):
            w = W[:, k]
            ss = (w * w).sum()
            if ss == 0:
                continue
            a = L[k, k]
            r = np.sqrt(a * a + ss)
            v0 = -ss / (a + r)
            iv = 1 / v0
            u = w * iv
            tau = -v0 / r
            L[k, k] = r
            beta[k] += 1.01 * rho * float(r)
            if k + 1 >= n1:
                continue
            rows = slice(k + 1, n1)
            l, Wr = L[rows, k], W[:, rows]
            beta[rows] += cstep * np.sqrt(f(l) ** 2 + f((Wr * Wr).sum(0)))
            s = (l + u @ Wr) * tau
            L[rows, k] = l - s
            W[:, rows] = Wr - np.outer(u, s)
        W[:, kb:ke] = Wk
    return L, W, beta


def remove_residual(L0, W0, L1, W1, kb0, kb1, n1, beta):
    """The orthogonal invariant of the steps kb0 .. kb1, and the bound an fp64 evaluation in any order keeps it to.

    Z = [L0[:, kb0 : kb1 + 128] | W0^T] on the rows kb0 <= i < n1 goes to Z' = [L1[:, same] | W1^T] with the w of every
    row inside the steps' blocks annihilated (taken as zero: the kernel leaves those rows of W as it found them), by a
    product of reflectors: Z' Z'^T = Z Z^T.  Returns (R, B): R = Z' Z'^T - Z Z^T in long double and the bound |R| <= B.

    The bound (Higham, chapter 19, row-wise).  Step k computes u^ and tau^ from row k as it finds it, (a, w^_k), each to a
    relative rho = 1.5 gamma_(mw + 8) (ss: mw fmas on non-negative terms; a^2 + ss; sqrt; a + r with a, r > 0; three
    quotients; one product), so the applied matrix is within 10 rho of the exact reflector H~ of (a, w^_k)
    (|tau^ |v^|^2 - 2| <= 3 rho (2), the unit direction within rho: its projector within 4 rho of the exact one).  Row i > k,
    x_i = (l_ik, w_i), becomes H~ x_i + f with |f|_2 <= (10 rho + 2 sqrt 2 gamma_mw + 3 u) |x_i|_2: the fma chain of s0
    errs by gamma_mw (|l| + |u| |w_i|), tau |v| (.) <= 2 sqrt 2 gamma_mw |x_i|; s = s0 tau, l - s and the fmas w - s u add
    u (2 + 1) |x_i|.  Row k ends as (r^, 0) = H~ x_k + f, |f| <= rho r.  The H~ are orthogonal, so the f of a row add up in
    norm without growing: beta_i = sum over the steps of these (1 % slack for the second-order terms; remove_blocks_ref
    accumulates it), computed Z' = (Z + D) Q with |D_i|_2 <= beta_i, and
        |R_ij| <= beta_i |z_j| + beta_j |z_i| + beta_i beta_j.
    (Bounds on the ELEMENTS of L' and W' against the long-double run cannot be had this way: the direction of a reflector
    depends on w_k / |w_k|, an elementwise or norm-wise running bound grows by 1 + 2 |x_i| / |w_k| >= 3 per step, 3^128
    within one launch, where the true error does not grow.)"""
    cols = slice(kb0, min(kb1 + RB, L0.shape[1]))
    rows = slice(kb0, n1)
    done = min(kb1 + RB, n1)  # rows below `done` keep a w
    Z = np.hstack([np.tril(L0)[rows, cols].astype(LD), W0[:, rows].T.astype(LD)])
    W1z = W1[:, rows].T.astype(LD).copy()
    W1z[:done - kb0] = 0
    Z1 = np.hstack([np.tril(L1)[rows, cols].astype(LD), W1z])
    R = Z1 @ Z1.T - Z @ Z.T
    zn = np.sqrt((Z * Z).sum(1)).astype(np.float64)
    b = beta[rows]
    B = (np.outer(b, zn) + np.outer(zn, b) + np.outer(b, b)) * _INFLATE
    return R, B, float(np.abs(Z @ Z.T).max())


@functools.lru_cache(maxsize=None)
def remove_problem(n1, mc, mw, cb0, single=False):
    """(Lt, W (mw x 512, zero-padded from mc), Lw, Ww, beta) of the block loop from cb0 (single: the step kb = cb0 alone)
    on the operands of this shape; every column of W is zero above row cb0."""
    Lt, W = remove_operands(n1, mc, zero_top=cb0)
    Wp = np.zeros((mw, Lt.shape[0]))
    Wp[:mc] = W
    kb1 = cb0 if single else (n1 - 1) // RB * RB
    return _frozen(Lt, Wp, *remove_blocks_ref(Lt, Wp, cb0, kb1, n1))


def commit_f64(prob, m, nslab, ev, c=C_EXACT, noise=NOISE_EXACT):
    """append_commit_kernel restated in float64, operation by operation (slab-order sums, right-looking Cholesky with
    sqrt, quotient and a - b c, forward substitution): (L22, z2, pivot or None)."""
    part = prob["part"].reshape(nslab, APPEND_PART)
    C = simil_exact(prob["X2"][:, 1], ev, c) + noise * np.eye(m)
    S = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            s = 0.0
            for q in range(nslab):
                s += part[q, i * 64 + j]
            S[i, j] = C[i, j] - s
    r = prob["y2"] - sum(part[q, 4096:4096 + m] for q in range(nslab))
    bad = None
    with np.errstate(all="ignore"):
        for j in range(m):
            d = S[j, j]
            if bad is None and not d > 0.0:
                bad = j
            l = np.sqrt(d)
            S[j, j] = l
            S[j + 1:, j] /= l
            for i in range(j + 1, m):
                S[i, j + 1:i + 1] -= S[i, j] * S[j + 1:i + 1, j]
    if bad is not None:
        return None, None, bad
    for j in range(m):
        r[j] = r[j] / S[j, j]
        r[j + 1:] -= S[j + 1:, j] * r[j]
    return np.tril(S), r, None


# ---- the cases the GPU tests and their CPU self-checks share -------------------------------------------------------------
GRAM_M = (1, 2, 4, 8, 15, 16, 17, 32, 33, 34, 36, 40, 48, 64)
#: (npc, npc - n, m, ROWS layout)
GRAM_CASES = ([(npc, dn, m, False) for npc in (256, 768) for dn in (0, 3, 255) for m in GRAM_M]
              + [(npc, 3, m, True) for npc in (256, 768) for m in (1, 17, 64)])
COMMIT_CASES = [(m, nslab, n, ev) for m in (1, 5, 16, 17, 64) for nslab in (1, 3) for n in (0, 300) for ev in (False, True)]
#: (m, pivot, how)
NOTPD_CASES = [(m, p, how) for m in (5, 64) for p, how in ((0, "zero"), (m // 2, "neg"), (m - 1, "zero"), (m // 2, "nan"))]
#: (K, ncols, ldb, tri, sub)
PANEL_SHAPES = [(256, 256, 256, True, False), (1024, 1024, 1280, True, False), (256, 64, 1280, False, True),
                (256, 768, 1280, False, True), (1024, 256, 1280, False, True)]
PANEL_ROWS16 = (1, 2, 3, 4, 5, 9)
#: (m, npad or None: Vt NULL, ncu, mo, ev) -> what the case reaches
PCOV_CASES = [
    (65, 1280, 1, 65, False),      # two slabs of 768 and 512 columns
    (65, 1280, 256, 65, False),    # five slabs
    (1, 2048, 256, 1, False),      # nslab = 8: the 8-wide sum alone
    (17, 2048, 256, 17, False),
    (1, 2560, 256, 1, False),      # nslab = 10: 8 + a tail of 2
    (17, 2560, 256, 17, False),
    (130, 256, 256, 130, False),   # off-diagonal tile pairs
    (70, 256, 256, 128, False),    # mo = 128: the identity padding
    (65, None, 256, 65, False),    # Vt NULL: the prior Gram matrix
    (70, None, 256, 128, True),
    (65, 1280, 256, 65, True),     # events, points on both sides of a boundary
]
PCOV_SLABS = {(65, 1280, 1): (2, 768), (65, 1280, 256): (5, 256), (1, 2048, 256): (8, 256), (17, 2560, 256): (10, 256)}
REMOVE_N1 = (100, 128, 129, 385, 512)
#: (n1, mw, mc, cb0, single step)
REMOVE_CASES = ([(n1, mw, mc, 0, False) for n1 in REMOVE_N1 for mw, mc in ((4, 1), (4, 4), (32, 5), (32, 32))]
                + [(n1, 32, mc, 0, False) for n1 in (129, 512) for mc in (1, 4)]  # the wide instance on the narrow one's m
                + [(n1, mw, mw, 128, False) for n1 in (385, 512) for mw in (4, 32)]
                + [(100, 4, 1, 0, True), (385, 4, 4, 0, True), (385, 32, 32, 128, True), (512, 32, 5, 384, True)])
TWO_PASS = (385, 33)  # n1, m: a pass of 32 columns, then one of a single column
