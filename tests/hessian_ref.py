"""The Hessian of the LML in the log hyperparameters (gogp_lml_hessian): the numpy reference its tests share, in
np.longdouble and without any second derivative of the kernel.

The analytic gradient 1/2 tr(W K_p), W = alpha alpha^T - K^-1, from the descriptor evaluation the other references
have (gram_ref.pair_values for K, grad_reduce_ref.slot_sums / assemble for the sums over W) on a long-double Cholesky
inverse, is differentiated by central differences in log theta at the steps h = 1e-3 and h / 2 and Richardson-
extrapolated.  The tolerance of a comparison comes from the reference alone: entrywise 10 |H(h) - H(extrapolated)|, the
truncation the extrapolation removed, plus 1e-9 max|H| for the fp64 arithmetic of the device.

Beside it (below `hessian`): the closed-form first and second derivatives of all five kinds in the logs of their parameters
(`Term`), the Hessian straight from them per parameter (`analytic`, in long doubles or restated in float64), and what each
kernel of csrc/hessian.hip returns from the inputs a hook is handed (`kernel_inputs`, `slot_matrices`, `moments`), over the
descriptor space ALL_CASES.  CASES stays the three descriptors of the Richardson test.
"""
import numpy as np

import gram_ref as GR
import grad_reduce_ref as G
from gogp_amd import kernel
from handle_state_ref import inputs

LD = np.longdouble
H_STEP = 1e-3

#: name -> (NDim, similarity, noise, theta): the three descriptors of the tests
CASES = {
    "ard": (3, kernel.Scaled(kernel.ARD(kernel.Normal, 3)), kernel.UniformNoise, [1.0, 0.7, 0.9, 1.3, 0.1]),
    "sum": (1, kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))]),
            kernel.ConstantNoiseParam(0.1), [1.0, 0.6, 0.5, 0.8, 0.07, 0.3]),
    "matern32": (2, kernel.Scaled(kernel.Matern32), kernel.UniformNoise, [1.2, 0.6, 0.15]),
}


#: CASES (the three the Richardson test walks at three sizes) and the descriptor space below
ALL_CASES = dict(CASES)

# ---- the descriptor space (tests/test_hessian_kernels.py, the analytic tests of tests/test_hessian_gpu.py): every radial
# kind scaled and unscaled at D = 1, 2 with the four noise kernels in turn; ARD at D = 3 (above: "ard"), 9 (S = 10 slots: 65
# trace pairs, two launches) and 4 (groups of 3 + 2, the second starting on an ARD slot); ARD(Periodic) against the period;
# an unscaled periodic term; four terms; the permuted parameter layout [c1, c2, l1, l2, p] of the hyperpriors tutorial.
# Lengths of the order of the inputs' spread and a noise of 0.2 .. 0.5 keep K well conditioned: the float64 restatement
# stays within 1e-10 of the long-double one (tests/test_hessian_ref_cpu.py).
_RADIAL = {"normal": kernel.Normal, "matern32": kernel.Matern32, "matern52": kernel.Matern52, "matern52tb": kernel.Matern52Textbook}
_NOISES = [(kernel.UniformNoise, [0.3]), (kernel.ConstantNoise(0.4), []), (kernel.ConstantNoiseParam(0.35), [0.3]),
           (kernel.ScaledNoise(0.5), [0.45])]
for _i, (_k, _obj) in enumerate(_RADIAL.items()):
    for _j, _D in enumerate((1, 2)):
        _no, _tn = _NOISES[(_i + _j) % 4]
        ALL_CASES["%s-s-D%d" % (_k, _D)] = (_D, kernel.Scaled(_obj), _no, [1.1 + 0.1 * _i, 0.7 + 0.2 * _j] + _tn)
        _no, _tn = _NOISES[(_i + _j + 2) % 4]
        ALL_CASES["%s-u-D%d" % (_k, _D)] = (_D, _obj, _no, [0.8 + 0.15 * _j] + _tn)
ALL_CASES.update({
    "ard9": (9, kernel.Scaled(kernel.ARD(kernel.Normal, 9)), kernel.UniformNoise,
             [1.2] + [2.0 + 0.25 * d for d in range(9)] + [0.3]),
    "ard-m52-D4": (4, kernel.Scaled(kernel.ARD(kernel.Matern52, 4)), kernel.ScaledNoise(0.5), [1.3, 1.4, 1.9, 1.6, 2.2, 0.5]),
    "ard-periodic": (2, kernel.Scaled(kernel.ARD(kernel.Periodic, 2)), kernel.UniformNoise, [0.9, 1.1, 1.6, 2.7, 0.3]),
    "periodic-u-D1": (1, kernel.Periodic, kernel.ConstantNoise(0.4), [1.2, 2.3]),
    "four": (3, kernel.Sum([kernel.Scaled(kernel.Normal), kernel.Scaled(kernel.Matern32), kernel.Scaled(kernel.Matern52Textbook),
                            kernel.Scaled(kernel.Periodic)]), kernel.UniformNoise,
             [0.7, 1.4, 1.1, 2.2, 0.4, 0.9, 0.25, 1.1, 2.4, 0.3]),
    "hyperpriors": (2, kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))],
                                  order=[0, 2, 1, 3, 4]), kernel.ConstantNoiseParam(0.3), [1.0, 0.6, 0.9, 1.2, 0.31, 0.2]),
    "variances": (2, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, [1.2, 0.8, 0.25]),
    "duplicates": (2, kernel.Scaled(kernel.Matern32), kernel.UniformNoise, [1.1, 0.9, 0.3]),
})
NEW_CASES = tuple(k for k in ALL_CASES if k not in CASES)
NMAX = 200
#: the seed of each case's rows: fixed per name, so that a case added or renamed later moves no other case's data (and none
#: of the ratios DESIGN.md records)
SEEDS = {"ard-m52-D4": 1, "ard-periodic": 2, "ard9": 3, "duplicates": 4, "four": 5, "hyperpriors": 6, "matern32-s-D1": 8,
         "matern32-s-D2": 9, "matern32-u-D1": 10, "matern32-u-D2": 11, "matern52-s-D1": 12, "matern52-s-D2": 13,
         "matern52-u-D1": 14, "matern52-u-D2": 15, "matern52tb-s-D1": 16, "matern52tb-s-D2": 17, "matern52tb-u-D1": 18,
         "matern52tb-u-D2": 19, "normal-s-D1": 20, "normal-s-D2": 21, "normal-u-D1": 22, "normal-u-D2": 23,
         "periodic-u-D1": 24, "variances": 26}
assert set(SEEDS) == set(NEW_CASES) and len(set(SEEDS.values())) == len(SEEDS)


def data(name, n):
    """(D, simil, noise, X, y, x = log theta) of one case at n rows: the leading coordinates of handle_state_ref.inputs for
    the first three cases, the first n of NMAX seeded rows for the others ("duplicates": rows 7 and 20 repeat rows 3 and 11)."""
    D, simil, noise, theta = ALL_CASES[name]
    if name in CASES:
        c = inputs(n)
        return D, simil, noise, np.ascontiguousarray(c.X[:, :D]), c.y, np.log(np.array(theta))
    rng = np.random.default_rng([2861, SEEDS[name]])
    X = rng.uniform(-1.5, 1.5, (NMAX, D))
    y = np.sin(1.3 * X.sum(1)) + 0.3 * rng.standard_normal(NMAX)
    if name == "duplicates":
        X[7], X[20] = X[3], X[11]
    return D, simil, noise, np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n]), np.log(np.array(theta))


def variances(name, n):
    """The per-observation noise variances of a case: None but for "variances"."""
    if name != "variances":
        return None
    return 0.05 + 0.1 * np.random.default_rng(2879).uniform(size=NMAX)[:n]


def inverse(K):
    """K^-1 of a symmetric positive definite long-double matrix, by its Cholesky factor."""
    n = len(K)
    L, Li = np.zeros_like(K), np.zeros_like(K)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    for i in range(n):
        Li[i, i] = 1 / L[i, i]
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li.T @ Li


def parts(desc, x, X, y, v=None, mode="ld"):
    """(kp, K^-1, alpha) at x = log theta, long doubles (mode "f64": the same in float64); v: per-observation variances."""
    dt = LD if mode == "ld" else np.float64
    th = np.exp(np.asarray(x, float))
    kp = G.kp_from_desc(desc, th[:desc.ntheta_simil], th[desc.ntheta_simil:])
    K = GR.pair_values(kp, X, X, mode, diag_noise=True)[0]
    if v is not None:
        K = K + np.diag(np.asarray(v, float).astype(dt))
    Kinv = inverse(K)
    return kp, Kinv, Kinv @ y.astype(dt)


def gradient(desc, x, X, y, v=None):
    kp, Kinv, alpha = parts(desc, x, X, y, v)
    slots = G.slot_sums(kp, X, len(X), alpha, [Kinv])[0][0]
    return G.assemble(desc, slots, kp.dnoise)


_CACHE = {}


def hessian(name, n):
    """(H, tol) of one case, both (P, P) float64, computed once."""
    if (name, n) not in _CACHE:
        D, simil, noise, X, y, x = data(name, n)
        desc = kernel.build_desc(D, simil, noise)
        v = variances(name, n)

        def diff(h):
            rows = []
            for p in range(len(x)):
                e = np.zeros(len(x))
                e[p] = h
                rows.append((gradient(desc, x + e, X, y, v) - gradient(desc, x - e, X, y, v)) / (2 * LD(h)))
            return np.array(rows)

        d1, d2 = diff(H_STEP), diff(H_STEP / 2)
        H = (4 * d2 - d1) / 3
        tol = 10 * np.abs(d1 - H) + 1e-9 * np.abs(H).max()
        _CACHE[name, n] = (H.astype(np.float64), tol.astype(np.float64))
    return _CACHE[name, n]


# ---- closed forms: the first and second derivatives of every term in the LOG of its parameters --------------------------
# Written from the kernels' formulas (gogp_amd/kernel.py: _term_value), not from csrc/hess_eval.h.  A term is c F(S):
#   radial kinds   S = s = sum_d u_d^2, u_d = (xa_d - xb_d) / l_d; F = f(s), by the chain rule through r = sqrt(s):
#                  f' = f_r / (2 r), f'' = (f_rr - f_r / r) / (4 s).  d s / dlog l_d = -2 u_d^2, d2 s / dlog l_d^2 = 4 u_d^2,
#                  mixed 0 (one length for all dimensions: the sums over d).
#   periodic       S = sum_d sin^2(phi_d) / l_d^2, phi_d = pi |xa_d - xb_d| / (mult p); F = exp(-2 S), F' = -2 F, F'' = 4 F.
#                  dphi / dlog p = -phi:  dS/dlog p = -sum phi sin(2 phi) / l^2,  d2S/dlog p^2 = sum (phi sin 2 phi + 2 phi^2
#                  cos 2 phi) / l^2,  d2S/dlog p dlog l_d = 2 phi_d sin(2 phi_d) / l_d^2,  dS/dlog l_d = -2 sin^2 phi_d / l_d^2.
#   the scale c    d/dlog c of anything of the term is that thing.
# With S_a, S_ab the derivatives of S:  k_a = c F' S_a,  k_ab = c (F'' S_a S_b + F' S_ab).
# f'' of Matern-3/2 and of the reference's Matern-5/2 (coefficient 1) grows like 1 / r and only ever multiplies S_a S_b =
# O(r^4): the product is 0 at r = 0, which is the value taken here (the stated limit).
VALUE, LEN, ARD, PERIOD = 0, 1, 2, 3
HESS_G, HESS_NMOM = 3, 25


def _radial2(kind, s, dt):
    """f, f', f'' in s = r^2 (f'' 0 where s == 0 for the kinds whose f'' is singular there)."""
    if kind == G.K_NORMAL:
        e = np.exp(-s / 2)
        return e, -e / 2, e / 4
    a = dt(G.SQRT3 if kind == G.K_MATERN32 else G.SQRT5)
    r = np.sqrt(s)
    pos = s > 0
    ir = np.divide(1, r, out=np.zeros_like(r), where=pos)
    e = np.exp(-a * r)
    if kind == G.K_MATERN32:
        return (1 + a * r) * e, -(a * a / 2) * e, (a * a * a / 4) * e * ir
    q = dt(1) if kind == G.K_MATERN52 else dt(5) / dt(3)
    f1 = (q - a * a / 2 - a * q * r / 2) * e
    f2 = ((a * a * a / 2 - 3 * a * q / 2) * ir / 2 + a * a * q / 4) * e
    return (1 + a * r + q * s) * e, f1, np.where(pos, f2, 0) if kind == G.K_MATERN52 else f2


class Term:
    """One term on the pairs of the rows of X: F = c F(S), F1 = c F', F2 = c F'' (n x n) and S_of(type, dim)."""

    def __init__(self, kp, t, X, dt):
        T, D = kp.terms[t], kp.ndim
        c, il, Xd = dt(T["c"]), T["inv_len"].astype(dt), np.asarray(X, np.float64).astype(dt)
        dx = [Xd[:, None, d] - Xd[None, :, d] for d in range(D)]
        self.zero = np.zeros((len(Xd), len(Xd)), dt)
        self.periodic = T["kind"] == G.K_PERIODIC
        if not self.periodic:
            self.sd = [(dx[d] * il[d]) ** 2 for d in range(D)]
            self.S = sum(self.sd)
            f, f1, f2 = _radial2(T["kind"], self.S, dt)
        else:
            phi = [dt(T["w"]) * np.abs(dx[d]) for d in range(D)]
            self.sd = [(np.sin(phi[d]) * il[d]) ** 2 for d in range(D)]
            self.pd = [phi[d] * np.sin(2 * phi[d]) * il[d] ** 2 for d in range(D)]
            self.qd = [(phi[d] * np.sin(2 * phi[d]) + 2 * phi[d] ** 2 * np.cos(2 * phi[d])) * il[d] ** 2 for d in range(D)]
            self.S = sum(self.sd)
            f = np.exp(-2 * self.S)
            f1, f2 = -2 * f, 4 * f
        self.F, self.F1, self.F2 = c * f, c * f1, c * f2

    def S_of(self, type, dim):
        """(S_a, S_aa, S_pa) of a parameter: the derivative of S in its log, the second one, the mixed one with the period."""
        if type == VALUE:
            return self.zero, self.zero, self.zero
        if type == PERIOD:
            return -sum(self.pd), sum(self.qd), self.zero
        q = self.S if type == LEN else self.sd[dim]
        return -2 * q, 4 * q, (2 * (sum(self.pd) if type == LEN else self.pd[dim]) if self.periodic else self.zero)

    def first(self, a):
        return self.F if a[0] == VALUE else self.F1 * self.S_of(*a)[0]

    def second(self, a, b):
        """The second derivative in the parameters a, b = (type, dim) of this term."""
        if a[0] == VALUE:
            return self.first(b)
        if b[0] == VALUE:
            return self.first(a)
        Sa, Saa, Spa = self.S_of(*a)
        Sb, _, Spb = self.S_of(*b)
        Sab = Saa if a == b else (Spb if a[0] == PERIOD else (Spa if b[0] == PERIOD else self.zero))
        return self.F2 * Sa * Sb + self.F1 * Sab


def roles(desc):
    """param index -> (term, type, dim) for the similarity parameters (each occurs once in these descriptors)."""
    out = {}
    for t in range(desc.nterms):
        T = desc.terms[t]
        if T.scale_idx >= 0:
            out[T.scale_idx] = (t, VALUE, 0)
        if T.ard:
            for j in range(desc.ndim):
                out[T.len_idx + j] = (t, ARD, j)
        else:
            out[T.len_idx] = (t, LEN, 0)
        if T.kind == G.K_PERIODIC:
            out[T.period_idx] = (t, PERIOD, 0)
    assert sorted(out) == list(range(desc.ntheta_simil))
    return out


def slots(desc):
    """The slots in the order gogp_lml_hessian walks them, and their groups: ([(term, type, dim, param)], [(term, first, n)])."""
    sl, gr = [], []
    for t in range(desc.nterms):
        T = desc.terms[t]
        first = len(sl)
        if T.scale_idx >= 0:
            sl.append((t, VALUE, 0, T.scale_idx))
        if T.ard:
            sl += [(t, ARD, j, T.len_idx + j) for j in range(desc.ndim)]
        else:
            sl.append((t, LEN, 0, T.len_idx))
        if T.kind == G.K_PERIODIC:
            sl.append((t, PERIOD, 0, T.period_idx))
        gmax = 2 if T.kind == G.K_PERIODIC else HESS_G
        gr += [(t, q, min(gmax, len(sl) - q)) for q in range(first, len(sl), gmax)]
    return sl, gr


def trace_pairs(S):
    """The pair list of gogp_lml_hessian: (a, b), a <= b < S, then (-1, b)."""
    return [(a, b) for a in range(S) for b in range(a, S)] + [(-1, b) for b in range(S)]


_ANALYTIC, _INPUTS, _SUMMANDS = {}, {}, {}  # (name, n, mode) -> (H, mag); (name, n) -> the hooks' inputs; -> summand_magnitudes


def analytic(name, n, v=None, mode="ld"):
    """(H, mag): the P x P Hessian straight from H_ij = 1/2 tr(W K_ij) - (K_i alpha)^T K^-1 (K_j alpha) + 1/2 tr(K^-1 K_i
    K^-1 K_j) per PARAMETER, the noise parameter (K_n = dnoise I, K_nn = 2 dnoise I) included, and the sum of the magnitudes
    of the three terms.  mode "f64": the same in float64.  v: per-observation variances (default: the case's)."""
    key = (name, n, mode)
    if v is None and key in _ANALYTIC:
        return _ANALYTIC[key]
    dt = LD if mode == "ld" else np.float64
    D, simil, noise, X, y, x = data(name, n)
    desc = kernel.build_desc(D, simil, noise)
    vv = variances(name, n) if v is None else v
    kp, Kinv, alpha = parts(desc, x, X, y, vv, mode)
    W = np.outer(alpha, alpha) - Kinv
    ns, nn = desc.ntheta_simil, 0 if desc.noise_kind == 0 else 1
    P = ns + nn
    terms = [Term(kp, t, X, dt) for t in range(desc.nterms)]
    rl = roles(desc)
    eye = np.eye(n, dtype=dt)
    Ki = [terms[rl[i][0]].first(rl[i][1:]) for i in range(ns)] + [dt(kp.dnoise) * eye] * nn
    Mi = [Kinv @ K for K in Ki]
    bi = [K @ alpha for K in Ki]
    H, mag = np.zeros((P, P), dt), np.zeros((P, P))
    for i in range(P):
        for j in range(i, P):
            if i < ns and j < ns:
                Kij = terms[rl[i][0]].second(rl[i][1:], rl[j][1:]) if rl[i][0] == rl[j][0] else None
            else:
                Kij = 2 * dt(kp.dnoise) * eye if i == j else None
            t1 = 0.5 * (W * Kij).sum() if Kij is not None else dt(0)
            t2 = bi[i] @ (Kinv @ bi[j])
            t3 = 0.5 * (Mi[i] * Mi[j].T).sum()
            H[i, j] = H[j, i] = t1 - t2 + t3
            mag[i, j] = mag[j, i] = float(abs(t1)) + float(abs(t2)) + float(abs(t3))
    if v is None:
        _ANALYTIC[key] = (H, mag)
    return H, mag


# ---- what the kernels of csrc/hessian.hip return, from the inputs a hook is handed ---------------------------------------
def kernel_inputs(name, n):
    """The inputs of the hooks for one case, computed once: the slots and groups, kp, X, and K^-1 and alpha of the long-double
    factorisation ROUNDED to float64 -- the numbers the device is given, which the references below take as exact."""
    key = (name, n)
    if key not in _INPUTS:
        D, simil, noise, X, y, x = data(name, n)
        desc = kernel.build_desc(D, simil, noise)
        kp, Kinv, alpha = parts(desc, x, X, y, variances(name, n))
        Kinv = Kinv.astype(np.float64)
        Kinv = np.tril(Kinv) + np.tril(Kinv, -1).T
        sl, gr = slots(desc)
        _INPUTS[key] = dict(D=D, desc=desc, kp=kp, X=X, Kinv=Kinv, alpha=alpha.astype(np.float64), slots=sl, groups=gr, n=n)
    return _INPUTS[key]


def slot_matrices(p, mode="ld"):
    """K_s = dK / dlog(slot s) for every slot, n x n."""
    dt = LD if mode == "ld" else np.float64
    terms = {}
    out = []
    for t, ty, dm, _ in p["slots"]:
        if t not in terms:
            terms[t] = Term(p["kp"], t, p["X"], dt)
        out.append(terms[t].first((ty, dm)))
    return out


def tile_sums(A, n, lower=True, npad=None):
    """The sums of the n x n array A over the 64-tiles of an npad x npad matrix (default: n rounded up): the lower ones row
    by row (lower) or all nt x nt."""
    nt = -(-n // 64) if npad is None else npad // 64
    pad = np.zeros((nt * 64, nt * 64), A.dtype)
    pad[:n, :n] = A
    t = pad.reshape(nt, 64, nt, 64).sum((1, 3))
    return np.array([t[i, j] for i in range(nt) for j in range(i + 1)]) if lower else t.reshape(-1)


def moments(p, t, ga, gb, mode="ld", npad=None):
    """hess_moments' layout for the groups ga, gb (lists of (type, dim)) of term t: (per lower 64-tile sums (ntl, 25), the
    tiles' sums of the magnitudes of the pairs' contributions (ntl, 25)).  Weight alpha_i alpha_j - Kinv_ij on j <= i, pairs
    off the diagonal twice."""
    dt = LD if mode == "ld" else np.float64
    n, a, T = p["n"], p["alpha"].astype(dt), Term(p["kp"], t, p["X"], dt)
    w = np.tril(np.outer(a, a) - p["Kinv"].astype(dt)) * (2 - np.eye(n, dtype=dt))
    nt = -(-n // 64) if npad is None else npad // 64
    ntl = nt * (nt + 1) // 2
    val, mag = np.zeros((ntl, HESS_NMOM), dt), np.zeros((ntl, HESS_NMOM))
    Sa = [T.S_of(*g) for g in ga]
    Sb = [T.S_of(*g) for g in gb]

    def put(idx, arr):
        val[:, idx] = tile_sums(w * arr, n, npad=npad)
        mag[:, idx] = tile_sums(np.abs(w * arr).astype(np.float64), n, npad=npad)

    G_ = HESS_G
    put(0, T.F)
    for q, s in enumerate(Sa):
        put(1 + q, T.F1 * s[0]), put(1 + 2 * G_ + q, T.F1 * s[1]), put(1 + 3 * G_ + q, T.F1 * s[2])
    for q, s in enumerate(Sb):
        put(1 + G_ + q, T.F1 * s[0]), put(1 + 4 * G_ + q, T.F1 * s[2])
    for qa, sa in enumerate(Sa):
        for qb, sb in enumerate(Sb):
            put(1 + 5 * G_ + qa * G_ + qb, T.F2 * sa[0] * sb[0])
    return val, mag


def summand_magnitudes(name, n):
    """(P, P): the magnitude of H_ij that an error of the device scales with, where analytic's `mag` has the magnitudes of
    the three sums.  Each term of H_ij is a sum of signed products (W = alpha alpha^T - K^-1 cancels, and so do the traces)
    whose factors come out of the factorisation -- alpha and K^-1, each with an error of its own -- and a product of m
    inexact factors errs by m times a factor's relative error to first order.  So every summand counts with its magnitude
    times the number of such factors in it:
        1/2 sum (2 |alpha_a alpha_b| + |K^-1_ab|) |K_ij,ab|        alpha alpha^T: two, K^-1: one
        3 sum |b_i,a K^-1_ab b_j,b|                                b = K_i alpha: one each, K^-1: one
        2 . 1/2 sum |M_i,ab M_j,ba|                                M = K^-1 K_i: one each
    b_i and M_i themselves are taken as the reference has them (their own inner sums are not opened)."""
    key = (name, n)
    if key in _SUMMANDS:
        return _SUMMANDS[key]
    dt = np.float64
    D, simil, noise, X, y, x = data(name, n)
    desc = kernel.build_desc(D, simil, noise)
    kp, Kinv, alpha = parts(desc, x, X, y, variances(name, n), "f64")
    W = 2 * np.abs(np.outer(alpha, alpha)) + np.abs(Kinv)
    ns, nn = desc.ntheta_simil, 0 if desc.noise_kind == 0 else 1
    P = ns + nn
    terms = [Term(kp, t, X, dt) for t in range(desc.nterms)]
    rl = roles(desc)
    eye = np.eye(n)
    Ki = [terms[rl[i][0]].first(rl[i][1:]) for i in range(ns)] + [kp.dnoise * eye] * nn
    Mi = [np.abs(Kinv @ K) for K in Ki]
    bi = [np.abs(K @ alpha) for K in Ki]
    out = np.zeros((P, P))
    for i in range(P):
        for j in range(i, P):
            if i < ns and j < ns:
                Kij = terms[rl[i][0]].second(rl[i][1:], rl[j][1:]) if rl[i][0] == rl[j][0] else None
            else:
                Kij = 2 * kp.dnoise * eye if i == j else None
            t1 = 0.5 * (W * np.abs(Kij)).sum() if Kij is not None else 0.0
            out[i, j] = out[j, i] = t1 + 3 * (bi[i] @ (np.abs(Kinv) @ bi[j])) + (Mi[i] * Mi[j].T).sum()
    _SUMMANDS[key] = out
    return out
