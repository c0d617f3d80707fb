"""Host reference of Vecchia's approximation on blocks of targets (gogp_amd/csrc/vecchia_blocks.hip; include/gogp_hip.h:
gogp_vecchia_blocks_*), written from the definition, not from the device code and not from its rank-t identity:

    value of block k = LML(C + T) - LML(C), two dense solves (the hand-written Cholesky of vecchia_ref, so that the same code
                       runs in float64 and numpy.longdouble);
    slots of block k = slots(alpha alpha^T - K^-1) on C + T minus the same on C, each K^-1 from solves against the identity;
    terms of target q = the sequential conditional of y_q on C and the block's earlier targets (vecchia_ref.block_terms on
                       the rows [C, T_0 .. T_q], a factorisation per target);
    produce           = k*^T K_C^-1 y_C and sqrt(k(z, z) - k*^T K_C^-1 k*) by dense solves."""
import numpy as np

import vecchia_ref as V

F64, LD = np.float64, np.longdouble


def _dense(kp, Xs, ys, vs, dt):
    """(LML, slot sums of alpha alpha^T - K^-1) of the rows given."""
    n = len(ys)
    if n == 0:
        return dt(0), np.zeros(V.NACC, dt)
    pairs = V.Pairs(kp, Xs, dt)
    L = V.cholesky(V.block_matrix(kp, Xs, vs, dt, pairs=pairs))
    z = V.forward(L, np.asarray(ys, F64).astype(dt))
    alpha = V.backward(L, z)
    eye = np.eye(n, dtype=dt)
    Kinv = np.stack([V.backward(L, V.forward(L, eye[:, j])) for j in range(n)], axis=1)
    Kinv = (Kinv + Kinv.T) / 2
    lml = -(z @ z) / 2 - np.log(np.diag(L)).sum() - n * np.log(2 * np.arccos(dt(-1))) / 2
    return lml, pairs.slots(np.outer(alpha, alpha) - Kinv)


def observe(kp, X, y, v, blocks, mode="ld"):
    """terms (N x 3), value, slots (NACC), the blocks' own contributions vblk (nb) and sblk (nb x NACC), failed (blocks with a
    bad pivot: NaN terms, nothing added)."""
    dt = LD if mode == "ld" else F64
    X, y = np.asarray(X, F64), np.asarray(y, F64)
    v = None if v is None else np.asarray(v, F64)
    tbl, nc, nt = blocks
    terms, failed = np.zeros((len(y), 3), dt), []
    vblk, sblk = np.zeros(len(nc), dt), np.zeros((len(nc), V.NACC), dt)
    for k in range(len(nc)):
        c, b = tbl[k, :nc[k]].astype(np.int64), tbl[k, :nc[k] + nt[k]].astype(np.int64)
        try:
            l1, s1 = _dense(kp, X[b], y[b], None if v is None else v[b], dt)
            l0, s0 = _dense(kp, X[c], y[c], None if v is None else v[c], dt)
            for q in range(nc[k], nc[k] + nt[k]):
                r = b[:q + 1]
                terms[b[q]] = V.block_terms(kp, X[r], y[r], None if v is None else v[r], dt, want_w=False)[:3]
        except V.NotPositive:
            failed.append(k)
            terms[b[nc[k]:]] = np.nan
            continue
        vblk[k], sblk[k] = l1 - l0, s1 - s0
    return dict(terms=terms, value=vblk.sum(), slots=sblk.sum(0), vblk=vblk, sblk=sblk, failed=failed)


def produce(kp, X, y, v, Z, offsets, groups, mode="ld"):
    dt = LD if mode == "ld" else F64
    X, y, Z = np.asarray(X, F64), np.asarray(y, F64), np.asarray(Z, F64)
    tbl, nc = groups
    mu, sigma = np.zeros(len(Z), dt), np.zeros(len(Z), dt)
    for g in range(len(nc)):
        c = tbl[g, :nc[g]].astype(np.int64)
        L = V.cholesky(V.block_matrix(kp, X[c], None if v is None else np.asarray(v, F64)[c], dt)) if len(c) else None
        for j in range(offsets[g], offsets[g + 1]):
            Kz = V.Pairs(kp, np.concatenate([X[c], Z[j:j + 1]]), dt).matrix()
            ks, prior = Kz[-1, :-1], Kz[-1, -1]
            if len(c):
                mu[j] = ks @ V.backward(L, V.forward(L, y[c].astype(dt)))
                prior = prior - ks @ V.backward(L, V.forward(L, ks))
            sigma[j] = np.sqrt(prior)
    return mu, sigma


def kernel_of(kind, D):
    """(similarity kernel object, natural parameters) of the families of tests/test_vecchia_kernel.py plus ARD: unit scale,
    lengths ~ sqrt(D)."""
    from gogp_amd import kernel as GK
    ln = 0.8 * float(np.sqrt(D))
    one = {"normal": GK.Normal, "matern32": GK.Matern32, "matern52": GK.Matern52, "matern52tb": GK.Matern52Textbook}
    if kind in one:
        return GK.Scaled(one[kind]), [1.3, ln]
    if kind == "ard":
        return GK.Scaled(GK.ARD(GK.Normal, D)), [1.2] + [ln * (1.0 + 0.1 * d) for d in range(D)]
    if kind == "max_terms":
        return (GK.Sum([GK.Scaled(GK.Normal), GK.Scaled(GK.Matern32), GK.Scaled(GK.Matern52Textbook), GK.Scaled(GK.Periodic)]),
                [0.7, ln, 1.1, 1.6 * ln, 0.4, 0.6 * ln, 0.25, 0.8 * ln, 0.45])
    return V.golden_kernel(kind, D)  # periodic, hyperpriors


def random_blocks(rng, shapes):
    """A valid table of the (c, t) shapes in the order given: consecutive targets, the conditioning rows drawn from the
    earlier ones in random order."""
    cond, targ, n = [], [], 0
    for c, t in shapes:
        assert c <= n
        cond.append(rng.choice(n, size=c, replace=False) if c else np.zeros(0, np.int64))
        targ.append(np.arange(n, n + t))
        n += t
    from gogp_amd import vecchia as VT
    return VT._pack(cond, targ, max(c + t for c, t in shapes)), n
