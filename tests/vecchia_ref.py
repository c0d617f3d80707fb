"""Host references of Vecchia's approximation (gogp_amd/csrc/vecchia.hip; include/gogp_hip.h: gogp_vecchia_*), written
from the formulas, not from the device code.  Target i with conditioning rows c (the table's order), q = |c|, block
b = [c..., i]:

    K_b = k(X_b, X_b) + diag(noise_var + v_b),  L = chol(K_b) (target last),  z = L^-1 y_b
    mu_i = y_i - L_qq z_q,   s_i = L_qq,   log p_i = -1/2 log 2 pi - log L_qq - 1/2 z_q^2
    alpha = L^-T z,  r = L^-T e_q,  e = z_q alpha - 1/2 (1 + z_q^2) r,  W = e r^T + r e^T
    d log p_i / d log theta_p = 1/2 sum_ab W_ab dK_ab / d log theta_p

(the rank-two identity K_b^-1 - pad(K_c^-1) = r r^T, alpha - pad(alpha_c) = z_q r).  Produce: the target row is the test
point with k(z, z) on its diagonal, no noise and no y: mu = sum_{t<q} L_qt z_t, sigma = L_qq.

`observe` / `produce` restate this with a hand-written Cholesky and substitutions in float64 (mode "f64") or
numpy.longdouble (mode "ld"); the kernel families, their parameter block and the slot sums of the pair reduction are
those of gram_ref / grad_reduce_ref.  `observe_dense` is a second reference that does NOT use the identity: term i is
LML(c + i) - LML(c) and its gradient the difference of the two dense gradients, from numpy's dense solves in float64
(tests/test_vecchia_cpu.py pins the first to it)."""
import numpy as np

import gram_ref as R
import grad_reduce_ref as G

F64, LD = np.float64, np.longdouble
NACC, ACC_TRACE = G.NACC, G.ACC_TRACE


class NotPositive(Exception):
    def __init__(self, pivot):
        super().__init__("pivot %d is not positive and finite" % pivot)
        self.pivot = pivot


def cholesky(K):
    """Lower factor of the lower triangle of K, left-looking, the sums in index order; NotPositive at the first pivot that
    is not positive and finite."""
    n = len(K)
    L = np.zeros_like(K)
    for j in range(n):
        s = K[j:, j] - L[j:, :j] @ L[j, :j] if j else K[j:, j].copy()
        d = s[0]
        if not (d > 0 and np.isfinite(d)):
            raise NotPositive(j)
        ljj = np.sqrt(d)
        L[j, j] = ljj
        L[j + 1:, j] = s[1:] / ljj
    return L


def forward(L, b):
    z = np.zeros_like(b)
    for i in range(len(b)):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    return z


def backward(L, b):
    """L^-T b."""
    x = np.zeros_like(b)
    for i in range(len(b) - 1, -1, -1):
        x[i] = (b[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


class Pairs:
    """The pairs (a, b), b <= a, of one block, each evaluated once: the values k_ab and, kept for `slots`, what the
    derivatives need.  The formulas are gram_ref.pair_values' and grad_reduce_ref._pair_terms' (their running-error
    bounds left out and the upper triangle not evaluated, which makes a block some five times cheaper);
    tests/test_vecchia_cpu.py pins both results to those two functions."""

    def __init__(self, kp, Xb, dt):
        self.kp, self.dt, self.n = kp, dt, len(Xb)
        self.ia, self.ib = np.tril_indices(self.n)
        X = np.asarray(Xb, F64).astype(dt)
        diff = [X[self.ia, d] - X[self.ib, d] for d in range(kp.ndim)]
        self.k, self.kept = np.zeros(len(self.ia), dt), []
        for T in kp.terms:
            c, il = dt(T["c"]), T["inv_len"].astype(dt)
            if T["kind"] != G.K_PERIODIC:
                u2 = [(diff[d] * il[d]) ** 2 for d in range(kp.ndim)]
                sq = sum(u2)
                f, f1, _ = G._radial(T["kind"], sq, dt)
                self.kept.append((c * f, -2 * c * f1 * sq, None, [-2 * c * f1 * u for u in u2] if T["ard"] else None))
            else:
                phi = [dt(T["w"]) * np.abs(diff[d]) for d in range(kp.ndim)]
                sn = [np.sin(q) for q in phi]
                dd2 = [(sn[d] * il[d]) ** 2 for d in range(kp.ndim)]
                gp = sum(sn[d] * np.cos(phi[d]) * phi[d] * il[d] ** 2 for d in range(kp.ndim))
                sq = sum(dd2)
                cf = c * np.exp(-2 * sq)
                self.kept.append((cf, 4 * cf * sq, 4 * cf * gp, [4 * cf * u for u in dd2] if T["ard"] else None))
            self.k = self.k + self.kept[-1][0]

    def matrix(self):
        K = np.zeros((self.n, self.n), self.dt)
        K[self.ia, self.ib] = self.k
        K[self.ib, self.ia] = self.k
        return K

    def slots(self, W):
        """The NACC slot sums for the symmetric weights W: off-diagonal pairs twice, the trace slot sum W_aa."""
        w = W[self.ia, self.ib] * np.where(self.ia == self.ib, 1, 2)
        out = np.zeros(NACC, self.dt)
        for t, (T, (scale, length, period, ard)) in enumerate(zip(self.kp.terms, self.kept)):
            out[3 * t] = (w * scale).sum()
            if period is not None:
                out[3 * t + 2] = (w * period).sum()
            if ard is None:
                out[3 * t + 1] = (w * length).sum()
            else:
                for d, a in enumerate(ard):
                    out[G.ACC_ARD0 + d] = (w * a).sum()
        out[ACC_TRACE] = np.trace(W)
        return out


def block_matrix(kp, Xb, vb, dt, produce=False, pairs=None):
    """K_b: the similarity plus noise_var + v on the diagonal (not on a Produce target, the last row)."""
    K = (pairs or Pairs(kp, Xb, dt)).matrix()
    add = np.full(len(Xb), kp.noise_var, F64) + (0.0 if vb is None else np.asarray(vb, F64))
    if produce:
        add[-1] = 0.0
    K[np.arange(len(Xb)), np.arange(len(Xb))] += add.astype(dt)
    return K


def block_terms(kp, Xb, yb, vb, dt, want_w=True):
    """(mu, s, logp, slot sums or None) of one block, the target last."""
    pairs = Pairs(kp, Xb, dt)
    K = block_matrix(kp, Xb, vb, dt, pairs=pairs)
    L = cholesky(K)
    y = np.asarray(yb, F64).astype(dt)
    z = forward(L, y)
    q = len(y) - 1
    lqq, zq = L[q, q], z[q]
    mu = y[q] - lqq * zq
    logp = -np.log(2 * np.arccos(dt(-1))) / 2 - np.log(lqq) - zq * zq / 2
    W = None
    if want_w:
        alpha = backward(L, z)
        eq = np.zeros(q + 1, dt)
        eq[q] = 1
        r = backward(L, eq)
        e = zq * alpha - (1 + zq * zq) / 2 * r
        W = pairs.slots(np.outer(e, r) + np.outer(r, e))
    return mu, lqq, logp, W


def slots_of(kp, Xb, W, dt):
    """The NACC slot sums of the block's pair reduction (off-diagonal pairs twice, the trace slot sum W_aa)."""
    n = len(Xb)
    vals, _ = G.slot_sums(kp, np.asarray(Xb, F64), n, np.zeros(n), [-W], mode="ld" if dt is LD else "f64")
    return vals[0]


def rows_of(nbr, i):
    r = np.asarray(nbr[i]) if nbr.shape[1] else np.zeros(0, np.int64)
    return r[r >= 0].astype(np.int64)


def observe(kp, X, y, v, nbr, mode="ld", grad=True, blocks=None):
    """terms (N x 3), value, slots (NACC), failed (list of targets with a bad pivot: NaN terms, nothing added) and, with
    `blocks`, the per-workgroup partial rows (blocks x NACC) and values (blocks): target i belongs to workgroup i % blocks."""
    dt = LD if mode == "ld" else F64
    X, y = np.asarray(X, F64), np.asarray(y, F64)
    N = len(y)
    terms = np.zeros((N, 3), dt)
    nb = blocks or 1
    part, vpart = np.zeros((nb, NACC), dt), np.zeros(nb, dt)
    failed = []
    for i in range(N):
        c = rows_of(nbr, i)
        b = np.concatenate([c, [i]])
        try:
            mu, s, logp, W = block_terms(kp, X[b], y[b], None if v is None else np.asarray(v, F64)[b], dt, grad)
        except NotPositive:
            failed.append(i)
            terms[i] = np.nan
            continue
        terms[i] = mu, s, logp
        vpart[i % nb] += logp
        if grad:
            part[i % nb] += W
    out = dict(terms=terms, value=vpart.sum(), slots=part.sum(0), failed=failed)
    if blocks:
        out.update(partials=part, vpart=vpart)
    return out


def produce(kp, X, y, v, Z, nbrz, mode="ld"):
    """(mu, sigma, failed) of the test points Z, each on the rows its row of nbrz names."""
    dt = LD if mode == "ld" else F64
    X, y, Z = np.asarray(X, F64), np.asarray(y, F64), np.asarray(Z, F64)
    mz = len(Z)
    mu, sigma, failed = np.zeros(mz, dt), np.zeros(mz, dt), []
    for j in range(mz):
        c = rows_of(nbrz, j)
        Xb = np.concatenate([X[c], Z[j:j + 1]])
        vb = None if v is None else np.concatenate([np.asarray(v, F64)[c], [0.0]])
        try:
            L = cholesky(block_matrix(kp, Xb, vb, dt, produce=True))
        except NotPositive:
            failed.append(j)
            mu[j] = sigma[j] = np.nan
            continue
        q = len(c)
        z = forward(L[:q, :q], y[c].astype(dt))
        mu[j] = L[q, :q] @ z
        sigma[j] = L[q, q]
    return mu, sigma, failed


# ---- the second reference: no rank-two identity ---------------------------------------------------------------------
def _dense(kp, Xs, ys, vs):
    """(LML, slot sums of W = alpha alpha^T - K^-1) of the rows given, by numpy's dense routines in float64."""
    n = len(ys)
    if n == 0:
        return 0.0, np.zeros(NACC)
    K = R.pair_values(kp, Xs, Xs, "f64")[0]
    K[np.arange(n), np.arange(n)] += kp.noise_var + (0.0 if vs is None else vs)
    sign, logdet = np.linalg.slogdet(K)
    assert sign > 0
    alpha = np.linalg.solve(K, ys)
    Kinv = np.linalg.solve(K, np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    lml = -0.5 * ys @ alpha - 0.5 * logdet - 0.5 * n * np.log(2 * np.pi)
    return lml, slots_of(kp, Xs, np.outer(alpha, alpha) - Kinv, F64)


def observe_dense(kp, X, y, v, nbr):
    """logp (N), value and slots (NACC) from LML(c + i) - LML(c) and the difference of the two dense gradients."""
    X, y = np.asarray(X, F64), np.asarray(y, F64)
    v = None if v is None else np.asarray(v, F64)
    N = len(y)
    logp, slots = np.zeros(N), np.zeros(NACC)
    for i in range(N):
        c = rows_of(nbr, i)
        b = np.concatenate([c, [i]])
        l1, s1 = _dense(kp, X[b], y[b], None if v is None else v[b])
        l0, s0 = _dense(kp, X[c], y[c], None if v is None else v[c])
        logp[i] = l1 - l0
        slots += s1 - s0
    return logp, logp.sum(), slots


# ---- tables and inputs of the tests ---------------------------------------------------------------------------------------
def random_table(rng, rows, m, n, causal=True, full=False):
    """A random table: per row a random number (full: as many as there are) of distinct indices, unsorted, then -1."""
    t = np.full((rows, m), -1, np.int32)
    for i in range(rows):
        lim = i if causal else n
        cap = min(m, lim)
        k = cap if full else int(rng.integers(0, cap + 1))
        if k:
            t[i, :k] = rng.choice(lim, size=k, replace=False)
    return t


def all_earlier(n):
    """Row i conditions on every earlier row: Vecchia is exact (n <= 64)."""
    t = np.full((n, max(n - 1, 0)), -1, np.int32)
    for i in range(n):
        t[i, :i] = np.arange(i)
    return t


def inputs(seed, N, D, span=3.0):
    """Inputs uniform on a few length scales (gram_ref.terms_of scales the lengths with sqrt(D)), y of unit scale."""
    rng = np.random.default_rng([211, seed, N, D])
    X = rng.uniform(-span, span, (N, D))
    y = np.sin(X.sum(1)) + 0.3 * rng.standard_normal(N)
    v = rng.uniform(0.0, 0.02, N)
    return X, y, v


#: the golden cases of tests/golden/vecchia.json (tools/make_vecchia_golden.py): name -> (kernel, D, N, m, table, with v)
GOLDEN = {}
for _N in (200, 1000):
    for _m in (7, 31, 63):
        GOLDEN["nearest-N%d-m%d" % (_N, _m)] = ("matern52", 3, _N, _m, "nearest", _m == 31)
        GOLDEN["previous-N%d-m%d" % (_N, _m)] = ("hyperpriors", 1, _N, _m, "previous", False)
for _k in ("normal", "matern32", "matern52", "periodic"):
    GOLDEN["exact-%s" % _k] = (_k, 2, 64, 63, "all", False)
GOLDEN_NOISE_STD = 0.12  # the parameter of UniformNoise (>= 0.05: well-conditioned blocks at unit scale)
GOLDEN_MZ = 65


def golden_kernel(kind, D):
    """(similarity kernel, natural parameters): unit scale, lengths ~ sqrt(D) so that the inputs span a few of them."""
    from gogp_amd import kernel as GK
    ln = 0.8 * float(np.sqrt(D))
    if kind == "periodic":
        return GK.Scaled(GK.Periodic), [0.9, 1.1, 2.6]
    if kind == "hyperpriors":  # c Matern-5/2 + c' Periodic with a scaled period (the hyperpriors tutorial's kernel)
        return GK.Sum([GK.Scaled(GK.Matern52), GK.Scaled(GK.PeriodScaled(GK.Periodic, 10.0))]), [1.0, 0.5 * ln, 1.3, ln, 0.6]
    return GK.Scaled({"normal": GK.Normal, "matern32": GK.Matern32, "matern52": GK.Matern52}[kind]), [1.3, ln]


def golden_problem(name):
    """A golden case from seeds: the kernel objects, x = log theta, the descriptor and its KP, X, y, v (or None), the
    table, the test points Z and their table."""
    import zlib
    from gogp_amd import kernel as GK
    from gogp_amd import vecchia as VT
    kind, D, N, m, table, with_v = GOLDEN[name]
    seed = zlib.crc32(name.encode()) & 0xffff
    simil, ts = golden_kernel(kind, D)
    tn = [GOLDEN_NOISE_STD]
    desc = GK.build_desc(D, simil, GK.UniformNoise)
    kp = G.kp_from_desc(desc, ts, tn)
    X, y, v = inputs(seed, N, D, span=2.0 if table == "all" else 3.0)
    if table == "previous":  # a time axis
        order = np.argsort(X[:, 0], kind="stable")
        X, y, v = X[order], y[order], v[order]
    rng = np.random.default_rng([223, seed])
    Z = rng.uniform(-2.0, 2.0, (GOLDEN_MZ, D))
    lengths = 1.0 / kp.terms[0]["inv_len"]
    if table == "nearest":
        t = VT.nearest(X, m, lengths)
    elif table == "previous":
        t = VT.previous(N, m)
    else:
        t = all_earlier(N)
    tz = VT.nearest_to(X, Z, m, lengths)
    return dict(name=name, D=D, N=N, m=m, simil=simil, noise=GK.UniformNoise, ts=ts, tn=tn, x=np.log(np.array(ts + tn)),
                desc=desc, kp=kp, X=X, y=y, v=(v if with_v else None), t=t, Z=Z, tz=tz)


def gradient_of(p, slots):
    """d value / d log theta of a golden problem from the slot sums (grad_reduce_ref.assemble)."""
    return G.assemble(p["desc"], slots, p["kp"].dnoise)
