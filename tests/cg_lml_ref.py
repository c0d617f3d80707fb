"""Numpy reference of the iterative exact GP's LML and gradient (gogp_cg_lml_gradient; include/gogp_hip.h states the
estimator; this file restates it from that text, not from the device code), shared by tests/test_cg_lml_cpu.py,
test_cg_grad_kernel.py, test_cg_lml_gpu.py and tools/make_cg_lml_golden.py.

    probes      z_s = D^1/2 (Ls xi1_s + xi2_s),  row s of Xi = [xi2 (N) | xi1 (r)]
    solves      K^ u_s = z_s by cg_ref's lock-step iteration; w_s = P^-1 z_s (the first preconditioned residual),
                rho0_s = z_s^T w_s, and every iteration's a and beta per column
    quadrature  T_kk = 1 / a_k + beta_{k-1} / a_{k-1},  T_{k,k+1} = sqrt(beta_k) / a_k,  k up to the column's count;
                quad_s = rho0_s e_1^T log(T_s) e_1 (dense eigh);  log|K^| = sum log D_i + log|C| + mean_s quad_s
    LML         -1/2 y^T alpha - 1/2 log|K^| - N/2 log 2 pi
    gradient    1/2 sum_ij W_ij dK^_ij / dlog theta,  W = alpha alpha^T - (1/t) sum_s u_s w_s^T,  through the pair
                derivatives of tests/grad_reduce_ref.py (slot sums, then its assemble)

cg_block_hist restates cg_ref.cg_block with the history kept and the element type a parameter; in float64 it returns
cg_ref.cg_block's bits (tests/test_cg_lml_cpu.py asserts it), so cg_ref stays the one statement of the iteration.  Modes:
"f64" is plain float64 throughout; "ld" runs the iteration, the probes and the reduction in numpy.longdouble (the
preconditioner's C^-1 and the tridiagonal's eigh stay float64: no long-double LAPACK), and slot_sums_ab returns beside the
long-double slot sums a running-error bound formed as grad_reduce_ref forms its bounds."""
import numpy as np

import cg_ref as C
import grad_reduce_ref as G
from gogp_amd import kernel as GK

LD, F64 = np.longdouble, np.float64
U = G.U


def form_probes(Ls, d, Xi, dt=F64):
    """Z (t, n): z_s = sqrt(d) o (Ls xi1_s + xi2_s) for the rows [xi2 | xi1] of Xi."""
    n, r = Ls.shape
    Xi = np.asarray(Xi, F64)
    z = Xi[:, :n].astype(dt)
    if r:
        z = z + Xi[:, n:n + r].astype(dt) @ Ls.T.astype(dt)
    return np.sqrt(np.asarray(d, F64).astype(dt)) * z


def apply_precond(P, Rb, dt=F64):
    """P^-1 Rb: cg_ref.Precond.apply itself in float64; in long double the same identity with C^-1 = inv(C) in float64."""
    if dt is F64:
        return P.apply(Rb)
    dis = P.dis.astype(dt)
    Rp = Rb * dis
    if P.G is None:
        return Rp * dis
    if not hasattr(P, "_cinv_ld"):
        P._cinv_ld = np.linalg.inv(P.C).astype(dt)
        P._ls_ld = P.Ls.astype(dt)
    return dis * (Rp - ((Rp @ P._ls_ld) @ P._cinv_ld) @ P._ls_ld.T)


def cg_block_hist(Kh, B, P, tol, max_iter, dt=F64):
    """cg_ref.cg_block with the history: dict(X, W = P^-1 B, rho0, a, beta (iterations x T; 0 for a frozen column),
    iterations, converged)."""
    B = np.asarray(B, F64).astype(dt)
    Kd = Kh if dt is F64 else Kh.astype(dt)
    T, n = B.shape
    x, r = np.zeros((T, n), dt), B.copy()
    bn = np.sqrt((B * B).sum(axis=1))
    frozen = bn == 0.0
    iters = np.zeros(T, dtype=np.int64)
    z = apply_precond(P, r, dt)
    w = z.copy()
    p = z.copy()
    rho = (r * z).sum(axis=1)
    rho0 = rho.copy()
    ah, bh = [], []
    for it in range(1, max_iter + 1):
        if frozen.all():
            break
        live = ~frozen
        q = p @ Kd
        pq = (p * q).sum(axis=1)
        if np.any(live & ~((pq > 0) & np.isfinite(pq))):
            raise C.NotPositiveDefinite(int(np.argmax(live & ~((pq > 0) & np.isfinite(pq)))))
        a = np.where(live, rho / np.where(live, pq, 1.0), 0.0)
        x[live] += a[live, None] * p[live]
        r[live] -= a[live, None] * q[live]
        rr = (r * r).sum(axis=1)
        iters[live] = it
        frozen = frozen | (live & (np.sqrt(rr) <= tol * bn))
        live = ~frozen
        z = apply_precond(P, r, dt)
        rho1 = (r * z).sum(axis=1)
        beta = np.where(live, rho1 / np.where(live, rho, 1.0), 0.0)
        p[live] = z[live] + beta[live, None] * p[live]
        rho = np.where(live, rho1, rho)
        ah.append(a)
        bh.append(beta)
    shape = (len(ah), T)
    return dict(X=x, W=w, rho0=rho0, a=np.array(ah, dt).reshape(shape), beta=np.array(bh, dt).reshape(shape),
                iterations=iters, converged=frozen.copy())


def tridiagonal(a, beta, m):
    """The m x m Lanczos tridiagonal of one column's coefficients a[0 .. m), beta[0 .. m - 1), in float64."""
    a, beta = np.asarray(a, LD), np.asarray(beta, LD)
    T = np.zeros((m, m))
    for k in range(m):
        T[k, k] = F64(1 / a[k] + (beta[k - 1] / a[k - 1] if k else 0))
        if k + 1 < m:
            T[k, k + 1] = T[k + 1, k] = F64(np.sqrt(beta[k]) / a[k])
    return T


def quadrature(a, beta, m, rho0):
    """rho0 e_1^T log(T) e_1 by a dense eigh; m == 0: 0."""
    if m < 1:
        return 0.0
    lam, V = np.linalg.eigh(tridiagonal(a, beta, m))
    return float(rho0) * float((V[0] ** 2 * np.log(lam)).sum())


def logdet_precond(P, d):
    ld = float(np.log(np.asarray(d, F64)).sum())
    return ld + (2.0 * float(np.log(np.diag(P.G)).sum()) if P.G is not None else 0.0)


def slot_sums_ab(kp, X, n, A, B, scale=1.0, mode="ld"):
    """(vals, bounds), NACC each: slot q = sum_{i, j < n} (scale sum_s A[s][i] B[s][j]) theta dk(x_i, x_j)/dtheta in the
    slot layout of grad_reduce_ref, the trace slot sum_i W_ii.  The bound is grad_reduce_ref's running-error bound of the
    pair sums at the weights W, and at the weights' own rounding gamma_{S+2} (|scale A|^T |B|) the same sums' magnitude
    (taken from the bound at those weights, which is at least gamma_m + 2 u times it)."""
    dt = LD if mode == "ld" else F64
    A, B = np.asarray(A, F64)[:, :n], np.asarray(B, F64)[:, :n]
    S = len(A)
    W = (scale * A).astype(dt).T @ B.astype(dt)
    Wabs = np.abs(scale * A).T @ np.abs(B)
    m = n * n
    acc = G._Acc([W, Wabs.astype(dt)], dt, (G.NACC,), m, n)
    G._pair_terms(kp, np.asarray(X, F64)[:n], n, acc, "diff", dt, False)
    g = G.gamma(m + 8) + 2 * U
    gs = G.gamma(S + 2)
    val, bnd = acc.val[0], acc.bnd[0] + gs * acc.bnd[1] / g
    tr = np.diag(W)
    val[G.ACC_TRACE] = tr.sum()
    bnd[G.ACC_TRACE] = ((G.gamma(n + 8) + 2 * U) * G._f64(tr).sum() + gs * np.diag(Wabs).sum()) * (1.0 + 2.0 ** -30)
    return val, bnd


def desc_of(p):
    return GK.build_desc(p["D"], p["simil"], C.NOISE)


def gradient_from(p, alpha, Us, Ws, mode="f64"):
    """d LML / d log theta = assemble(1/2 slots) of W = alpha alpha^T - (1/t) sum_s u_s w_s^T, and the slots' bound turned
    into the gradient's (assemble is linear with non-negative weights 1/2)."""
    t = len(Us)
    A = np.vstack([np.asarray(alpha)[None, :], -np.asarray(Us) / t])
    B = np.vstack([np.asarray(alpha)[None, :], np.asarray(Ws)])
    dt = LD if mode == "ld" else F64
    if mode == "ld":
        Wm = A.astype(dt).T @ B.astype(dt)
    else:
        Wm = A.T @ B
    n = p["N"]
    acc = G._Acc([Wm], dt, (G.NACC,), n * n, n)
    G._pair_terms(p["kp"], p["X"], n, acc, "diff", dt, False)
    acc.val[0][G.ACC_TRACE] = np.diag(Wm).sum()
    desc = desc_of(p)
    return G.assemble(desc, acc.val[0], 0.0), G.assemble(desc, acc.bnd[0], 0.0)


def estimate(p, rank, tol, Xi, max_iter=2000, piv_tol=0.0, mode="f64", gradient=True):
    """The whole estimator on one case of cg_ref (p = cg_ref.problem(name)): dict(lml, logdet, logdet_precond,
    logdet_stderr, quad, grad, iterations, converged, rank_used, alpha, yt_alpha)."""
    dt = LD if mode == "ld" else F64
    P, used = C.precond_of(p["K"], p["d"], rank, piv_tol)
    Xi = np.asarray(Xi, F64)
    t = len(Xi)
    sol = cg_block_hist(p["Kh"], p["y"][None, :], P, tol, max_iter, dt)
    alpha = sol["X"][0]
    Z = form_probes(P.Ls, p["d"], Xi, dt)
    # (a block's right-hand sides are float64 in every mode, as the device's are)
    blocks = [cg_block_hist(p["Kh"], np.asarray(Z[s0:s0 + C.MAX_RHS], F64), P, tol, max_iter, dt)
              for s0 in range(0, t, C.MAX_RHS)]
    quad, its, conv = [], [], []
    for b in blocks:
        for c in range(len(b["iterations"])):
            m = int(b["iterations"][c])
            quad.append(quadrature(b["a"][:m, c], b["beta"][:m, c], m, b["rho0"][c]))
        its += list(b["iterations"])
        conv += list(b["converged"])
    quad = np.array(quad)
    ldp = logdet_precond(P, p["d"])
    logdet = ldp + float(quad.mean())
    yta = float((p["y"].astype(dt) * alpha).sum())
    out = dict(lml=-0.5 * yta - 0.5 * logdet - 0.5 * p["N"] * np.log(2 * np.pi), logdet=logdet, logdet_precond=ldp,
               logdet_stderr=float(quad.std(ddof=1) / np.sqrt(t)) if t > 1 else 0.0, quad=quad,
               iterations=np.array(its), converged=np.array(conv), rank_used=used, alpha=np.asarray(alpha, F64), yt_alpha=yta)
    if gradient:
        Us = np.vstack([b["X"] for b in blocks])
        Ws = np.vstack([b["W"] for b in blocks])
        g, gb = gradient_from(p, alpha, Us, Ws, mode)
        out["grad"], out["grad_bound"] = np.asarray(g, F64), np.asarray(gb, F64)
        out["W"] = np.asarray(np.outer(alpha, alpha) - Us.T @ Ws / t, F64)
    return out


def dense(p):
    """The dense numpy values: dict(lml, logdet, grad) from slogdet, solve and 1/2 tr((alpha alpha^T - K^^-1) dK^)."""
    Kh, y, n = p["Kh"], p["y"], p["N"]
    sign, logdet = np.linalg.slogdet(Kh)
    assert sign > 0
    alpha = np.linalg.solve(Kh, y)
    Kinv = np.linalg.inv(Kh)
    Kinv = 0.5 * (Kinv + Kinv.T)
    vals, _ = G.slot_sums(p["kp"], p["X"], n, alpha, [Kinv], mode="ld")
    return dict(lml=float(-0.5 * y @ alpha - 0.5 * logdet - 0.5 * n * np.log(2 * np.pi)), logdet=float(logdet),
                grad=np.asarray(G.assemble(desc_of(p), vals[0], 0.0), F64), alpha=alpha, Kinv=Kinv)


def orthogonal_xi(n_total, seed):
    """sqrt(t) Q, Q a random orthogonal t x t matrix (t = n_total): (1/t) sum_s xi_s xi_s^T = I exactly up to rounding."""
    rng = np.random.default_rng([4242, n_total, seed])
    Q, _ = np.linalg.qr(rng.standard_normal((n_total, n_total)))
    return np.sqrt(n_total) * Q


#: the orthogonal-probe cases: name -> (base case of cg_ref, N, rank)
ORTHO = {"normal_1d": ("normal_1d", 96, 8), "matern32_1d": ("matern32_1d", 96, 0), "ard_8d": ("ard_8d", 120, 16),
         "periodic_matern_1d": ("periodic_matern_1d", 100, 8)}


def small_problem(name, N):
    """cg_ref.problem's case at its first N rows: X, v drawn as cg_ref.problem draws them, y from the prior at that N."""
    D, _, simil, theta, terms, (lo, hi) = C.CASES[name]
    rng = np.random.default_rng([20181, len(name), D, N])
    X = rng.uniform(lo, hi, (N, D))
    v = rng.uniform(0.0, 0.05, N)
    kp = G.KP(D, terms, noise_var=C.S2)
    K, Kh = C.khat_dense(kp, X, v)
    y = np.linalg.cholesky(Kh) @ rng.standard_normal(N)
    return dict(name=name, D=D, N=N, simil=simil, theta=np.array(theta, F64), x=np.log(np.array(theta, F64)), kp=kp, X=X, y=y,
                v=v, K=K, Kh=Kh, d=C.S2 + v, alpha=np.linalg.solve(Kh, y), cond=float(np.linalg.cond(Kh)))
