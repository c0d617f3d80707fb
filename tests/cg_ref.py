"""Numpy reference of the iterative exact GP (gogp_cg_*; include/gogp_hip.h states the formulas; this file restates them
from that text, not from the device code), shared by tests/test_cg_cpu.py, test_cg_kernels.py and test_cg_gpu.py.

    K^ = k(X, X) + s2 I + diag(v)
    preconditioner  P = L L^T + D,  D = diag(s2 + v_i),  L the N x r pivoted-Cholesky factor of k(X, X):
        d_i = K_ii;  step j: p = lowest index among the maximisers of d, stop unless d_p > tol;
        l_i = (K_ip - sum_{t<j} L[i][t] L[p][t]) / sqrt(d_p) (rows not yet selected), l_p = sqrt(d_p), 0 for rows selected
        earlier;  d_i -= l_i^2, d_p = 0
    Woodbury        Ls = D^-1/2 L,  C = I + Ls^T Ls,  P^-1 R = D^-1/2 (R' - Ls C^-1 Ls^T R'),  R' = D^-1/2 R
    lock-step CG    x = 0, r = b, z = P^-1 r, p = z, rho = r^T z;  per iteration: q = K^ p, a = rho / p^T q, x += a p,
                    r -= a q, a column FREEZES once |r| <= tol |b| (its count recorded, a = beta = 0 from then on),
                    z = P^-1 r, rho' = r^T z, beta = rho' / rho, p = z + beta p, rho = rho'

The kernel values and the error model of one element come from tests/gram_ref.py (pair_values); the product's bound is its
"matrix-vector row": gamma_n sum_j |K_ij V_tj| + sum_j e_ij |V_tj|, which holds for any order of the sum."""
import functools

import numpy as np

import gram_ref as R
from gogp_amd import kernel as GK
from grad_reduce_ref import KP, U, gamma

LD, F64 = np.longdouble, np.float64
_INFLATE = 1.0 + 2.0 ** -30
MAX_RHS, MAX_RANK = 64, 1024
S2 = 0.1 * 0.1  # the noise variance of every end-to-end case as the library forms it: ConstantNoise(0.1), std * std


# ---- the product ---------------------------------------------------------------------------------------------------------------
def kmm(kp, A, B, V, diag=None, mode="ld"):
    """(Out, bound): Out[t][i] = sum_j k(a_i, b_j) V[t][j] (+ diag_i V[t][i]; square only) and the bound of an fp64
    evaluation in any summation order.  A: (rows, D), B: (cols, D), V: (T, cols)."""
    dt = LD if mode == "ld" else F64
    k, e = R.pair_values(kp, A, B, mode)
    V = np.asarray(V, F64)
    mag = np.abs(R._f64(k))
    if diag is not None:
        assert k.shape[0] == k.shape[1]
        i = np.arange(len(k))
        k[i, i] += np.asarray(diag, F64).astype(dt)
        mag[i, i] += np.abs(diag)
        e[i, i] += U * mag[i, i] * _INFLATE  # the one rounding of k_ii + diag_i
    val = V.astype(dt) @ k.T
    n = k.shape[1]
    bound = gamma(max(n, 1)) * (np.abs(V) @ mag.T) + np.abs(V) @ e.T
    return val, bound * _INFLATE


def slab_columns(cols, nslab):
    """Per slab, the columns [a, b) launch_kmm gives it: ceil(tiles / nslab) tiles of 64 each, the last ones short or empty."""
    tiles = -(-cols // 64)
    tps = -(-tiles // nslab)
    return [(min(cols, s * tps * 64), min(cols, (s + 1) * tps * 64)) for s in range(nslab)]


def kmm_slabs(rows, cols):
    """The product's own number of slabs: about 2048 work items, a function of the sizes alone."""
    rt, ct = max(1, -(-rows // 64)), max(1, -(-cols // 64))
    return max(1, min(-(-2048 // rt), ct, 64))


# ---- preconditioner --------------------------------------------------------------------------------------------------------------
def pivoted_cholesky(K, rank, tol):
    """(L, piv): the N x m factor (m <= rank) of the recurrence above on the dense K (no noise)."""
    N = len(K)
    d = np.array(np.diag(K), F64)
    L = np.zeros((N, min(rank, N)))
    piv = []
    for j in range(min(rank, N)):
        p = int(np.argmax(d))
        if not d[p] > tol:
            break
        sq = np.sqrt(d[p])
        l = (K[:, p] - L[:, :j] @ L[p, :j]) / sq
        l[piv] = 0.0
        l[p] = sq
        L[:, j] = l
        d = d - l * l
        piv.append(p)
        d[piv] = 0.0
    return L[:, :len(piv)].copy(), np.array(piv, dtype=np.int64)


class Precond:
    """P^-1 by Woodbury's identity; L with no columns: Jacobi."""

    def __init__(self, L, d):
        self.dis = 1.0 / np.sqrt(d)
        self.Ls = L * self.dis[:, None]
        self.C = np.eye(L.shape[1]) + self.Ls.T @ self.Ls
        self.G = np.linalg.cholesky(self.C) if L.shape[1] else None

    def apply(self, Rb):
        Rp = Rb * self.dis
        if self.G is None:
            return Rp * self.dis
        W = Rp @ self.Ls
        Y = np.linalg.solve(self.G.T, np.linalg.solve(self.G, W.T)).T
        return self.dis * (Rp - Y @ self.Ls.T)


def precond_of(K, d, rank, piv_tol):
    L, _ = pivoted_cholesky(K, rank, piv_tol) if rank > 0 else (np.zeros((len(K), 0)), None)
    return Precond(L, d), L.shape[1]


# ---- lock-step CG ----------------------------------------------------------------------------------------------------------------
class NotPositiveDefinite(Exception):
    pass


def cg_block(Kh, B, P, tol, max_iter):
    """Solve Kh x_t = B[t] for the rows of B together.  Returns dict(X, iterations, converged, rel_residual,
    rel_residual_recurrence)."""
    B = np.asarray(B, F64)
    T, n = B.shape
    x, r = np.zeros((T, n)), B.copy()
    bn = np.sqrt((B * B).sum(axis=1))
    frozen = bn == 0.0
    iters = np.zeros(T, dtype=np.int64)
    rr = bn * bn
    z = P.apply(r)
    p = z.copy()
    rho = (r * z).sum(axis=1)
    for it in range(1, max_iter + 1):
        if frozen.all():
            break
        live = ~frozen
        q = p @ Kh
        pq = (p * q).sum(axis=1)
        if np.any(live & ~((pq > 0) & np.isfinite(pq))):
            raise NotPositiveDefinite(int(np.argmax(live & ~((pq > 0) & np.isfinite(pq)))))
        a = np.where(live, rho / np.where(live, pq, 1.0), 0.0)
        x[live] += a[live, None] * p[live]
        r[live] -= a[live, None] * q[live]
        rr[live] = (r[live] * r[live]).sum(axis=1)
        iters[live] = it
        frozen = frozen | (live & (np.sqrt(rr) <= tol * bn))
        live = ~frozen
        z = P.apply(r)
        rho1 = (r * z).sum(axis=1)
        beta = np.where(live, rho1 / np.where(live, rho, 1.0), 0.0)
        p[live] = z[live] + beta[live, None] * p[live]
        rho = np.where(live, rho1, rho)
    true = np.sqrt(((B - x @ Kh) ** 2).sum(axis=1))
    safe = np.where(bn > 0, bn, 1.0)
    return dict(X=x, iterations=iters, converged=frozen.copy(), rel_residual=np.where(bn > 0, true / safe, 0.0),
                rel_residual_recurrence=np.where(bn > 0, np.sqrt(rr) / safe, 0.0))


# ---- the end-to-end cases ----------------------------------------------------------------------------------------------------------
# name: (D, N, similarity kernel, natural parameters, the terms the device sees, box)
def _radial(kind, c, ell, D):
    return [dict(kind=kind, c=c, inv_len=1.0 / ell)]


_ARD_L = 1.5 + 0.25 * np.arange(8)
CASES = {
    "normal_1d": (1, 600, GK.Scaled(GK.Normal), [1.5, 0.5], _radial(R.K_NORMAL, 1.5, 0.5, 1), (0.0, 10.0)),
    "matern32_1d": (1, 600, GK.Scaled(GK.Matern32), [1.5, 0.5], _radial(R.K_MATERN32, 1.5, 0.5, 1), (0.0, 10.0)),
    "matern52_2d": (2, 600, GK.Scaled(GK.Matern52), [1.5, 0.7], _radial(R.K_MATERN52, 1.5, 0.7, 2), (0.0, 4.0)),
    "normal_3d": (3, 1000, GK.Scaled(GK.Normal), [1.5, 1.0], _radial(R.K_NORMAL, 1.5, 1.0, 3), (0.0, 4.0)),
    "periodic_matern_1d": (1, 500, GK.Sum([GK.Scaled(GK.Matern32), GK.Scaled(GK.Periodic)]), [1.5, 0.8, 0.5, 1.2, 2.5],
                           [dict(kind=R.K_MATERN32, c=1.5, inv_len=1.0 / 0.8),
                            dict(kind=R.K_PERIODIC, c=0.5, inv_len=1.0 / 1.2, w=np.pi / 2.5)], (0.0, 10.0)),
    "ard_8d": (8, 600, GK.Scaled(GK.ARD(GK.Normal, 8)), [1.5] + list(_ARD_L),
               [dict(kind=R.K_NORMAL, c=1.5, ard=True, inv_len=1.0 / _ARD_L)], (0.0, 4.0)),
    "normal_8d_4097": (8, 4097, GK.Scaled(GK.Normal), [1.5, 2.0], _radial(R.K_NORMAL, 1.5, 2.0, 8), (0.0, 4.0)),
}
TABULATED = ["normal_1d", "matern32_1d", "matern52_2d", "normal_3d"]
MATERN = ["matern32_1d", "matern52_2d"]
SMALL = [c for c in CASES if CASES[c][1] <= 1000]
NOISE = GK.ConstantNoise(0.1)


def khat_dense(kp, X, v):
    K = R._f64(R.pair_values(kp, X, X, "f64")[0])
    return K, K + np.diag(S2 + v)


@functools.lru_cache(maxsize=None)
def problem(name):
    """The data and the dense reference of one case, computed once and read only: X, y, v, K (no noise), Kh, d, alpha
    (numpy.linalg.solve), cond (numpy.linalg.cond; for the SPD matrix of N = 4097 the ratio of the extreme eigenvalues,
    which is the same number) and the parameter block kp."""
    D, N, simil, theta, terms, (lo, hi) = CASES[name]
    rng = np.random.default_rng([20181, len(name), D, N])
    X = rng.uniform(lo, hi, (N, D))
    v = rng.uniform(0.0, 0.05, N)
    kp = KP(D, terms, noise_var=S2)
    K, Kh = khat_dense(kp, X, v)
    y = np.linalg.cholesky(Kh) @ rng.standard_normal(N)
    if N <= 1000:
        cond = float(np.linalg.cond(Kh))
    else:
        w = np.linalg.eigvalsh(Kh)
        cond = float(w[-1] / w[0])
    out = dict(name=name, D=D, N=N, simil=simil, theta=np.array(theta, F64), x=np.log(np.array(theta, F64)), kp=kp, X=X,
               y=y, v=v, K=K, Kh=Kh, d=S2 + v, alpha=np.linalg.solve(Kh, y), cond=cond)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_solve(name, rank, tol, max_iter=2000, piv_tol=0.0):
    """The reference's own run of the y column: (result dict of cg_block, rank_used)."""
    p = problem(name)
    P, used = precond_of(p["K"], p["d"], rank, piv_tol)
    return cg_block(p["Kh"], p["y"][None, :], P, tol, max_iter), used


def alpha_bound(p, rel_residual):
    """Condition 3: |alpha - alpha*| <= (cond rel_residual + cond n u) |alpha*|."""
    return (p["cond"] * rel_residual + p["cond"] * p["N"] * U) * float(np.linalg.norm(p["alpha"]))


def true_residual_ld(p, alpha):
    """(|y - K^ alpha| / |y| in long double, the matrix-vector bound of that residual divided by |y|)."""
    kp, X, n = p["kp"], p["X"], p["N"]
    val, bnd = kmm(kp, X, X, np.asarray(alpha, F64)[None, :], diag=p["d"])
    res = p["y"].astype(LD) - val[0]
    yn = float(np.linalg.norm(p["y"]))
    return float(np.sqrt((res * res).sum())) / yn, float(np.linalg.norm(bnd[0] + U * np.abs(R._f64(res)))) / yn
