"""Leave-block-out cross-validation (gogp_blockcv, gogp_blockcv_gradient): the numpy references its tests share.
Families, events, noise and inputs: those of tests/loo_ref.py.

The rows are cut into F consecutive blocks B_f = [start[f], start[f + 1]).  Two independent things:

  * brute_force: the definition.  For every block the process is refitted to the rows outside it with numpy.linalg and
    predicts the block jointly; none of the closed forms below is used:
        mu_B = K_Bo K_oo^-1 y_o,  Sigma_B = K_BB - K_Bo K_oo^-1 K_oB  (K carries the noise on its diagonal),
        logp_f = -1/2 (y_B - mu_B)^T Sigma_B^-1 (y_B - mu_B) - 1/2 log det Sigma_B - |B| / 2 log 2 pi;
  * closed_form: with Q = K^-1 from np.linalg.inv, alpha = Q y and, per block, Q_BB = C C^T (lower Cholesky),
    X = C^-1, w = X alpha_B, v_B = X^T w, Sigma_B = X^T X:
        mu_B = y_B - v_B,  sigma_i = sqrt((Sigma_B)_ii),  logp_f = -1/2 |w|^2 + sum_i log C_ii - |B| / 2 log 2 pi,
        d sum_f logp_f / d log theta_p = sum_ab W_ab dK_ab / d log theta_p,
        W = 1/2 (u alpha^T + alpha u^T) - 1/2 Q M Q,  v = the stacked v_B,  u = Q v,  M = blockdiag(Sigma_B + v_B v_B^T).
    sqrt_factor is the square root of M_B the device uses: S_B = X^T + gamma v_B w^T,
    gamma = (sqrt(1 + |w|^2) - 1) / |w|^2 (1/2 at w = 0), S_B S_B^T = M_B.
"""
import numpy as np

import loo_ref as LR

LOG_2PI = LR.LOG_2PI
MAX_BLOCK = 128


def starts(lengths):
    """start for blocks of the given lengths"""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def groups(start):
    """The Python mirror of gogp_blockcv_groups: consecutive blocks packed greedily, in order, into groups of at most
    128 columns; returns first (ngroups + 1 entries): group g holds the blocks first[g] .. first[g + 1] - 1."""
    start = np.asarray(start, dtype=np.int64)
    F = len(start) - 1
    if F <= 0:
        return np.zeros(1, dtype=np.int64)
    first, cols = [0], 0
    for f in range(F):
        ln = int(start[f + 1] - start[f])
        if cols + ln > MAX_BLOCK:
            first.append(f)
            cols = 0
        cols += ln
    return np.array(first + [F], dtype=np.int64)


def brute_force(K, y, start):
    """(mu, sigma, logp): F refits on the rows outside each block; mu, sigma per row, logp per block."""
    y = np.asarray(y, float)
    n, F = len(y), len(start) - 1
    mu, sigma, logp = np.zeros(n), np.zeros(n), np.zeros(F)
    for f in range(F):
        a, b = int(start[f]), int(start[f + 1])
        inb = np.zeros(n, dtype=bool)
        inb[a:b] = True
        o = ~inb
        Kbb = K[np.ix_(inb, inb)]
        if o.any():
            L = np.linalg.cholesky(K[np.ix_(o, o)])
            A = np.linalg.solve(L, K[np.ix_(o, inb)])
            m = A.T @ np.linalg.solve(L, y[o])
            Sig = Kbb - A.T @ A
        else:
            m, Sig = np.zeros(b - a), Kbb
        Sig = 0.5 * (Sig + Sig.T)
        r = y[a:b] - m
        mu[a:b] = m
        sigma[a:b] = np.sqrt(np.diag(Sig))
        _, ld = np.linalg.slogdet(Sig)
        logp[f] = -0.5 * r @ np.linalg.solve(Sig, r) - 0.5 * ld - 0.5 * (b - a) * LOG_2PI
    return mu, sigma, logp


def block_terms(Q, alpha, a, b):
    """(C, X, w, v) of the block [a, b) of Q"""
    C = np.linalg.cholesky(0.5 * (Q[a:b, a:b] + Q[a:b, a:b].T))
    X = np.linalg.inv(C)
    w = X @ alpha[a:b]
    return C, X, w, X.T @ w


def sqrt_factor(X, w, v):
    """S_B = X^T + gamma v w^T with S_B S_B^T = X^T X + v v^T"""
    w2 = float(w @ w)
    gamma = 0.5 if w2 == 0.0 else (np.sqrt(1.0 + w2) - 1.0) / w2
    return X.T + gamma * np.outer(v, w)


def closed_form(K, y, start, dK=None):
    """(mu, sigma, logp) and, with the list dK of derivative matrices, the gradient of sum(logp) (else None)."""
    y = np.asarray(y, float)
    n, F = len(y), len(start) - 1
    Q = np.linalg.inv(K)
    Q = 0.5 * (Q + Q.T)
    alpha = np.linalg.solve(K, y)
    mu, sigma, logp = np.zeros(n), np.zeros(n), np.zeros(F)
    v, M = np.zeros(n), np.zeros((n, n))
    for f in range(F):
        a, b = int(start[f]), int(start[f + 1])
        C, X, w, vb = block_terms(Q, alpha, a, b)
        Sig = X.T @ X
        mu[a:b] = y[a:b] - vb
        sigma[a:b] = np.sqrt(np.diag(Sig))
        logp[f] = -0.5 * w @ w + np.log(np.diag(C)).sum() - 0.5 * (b - a) * LOG_2PI
        v[a:b] = vb
        M[a:b, a:b] = Sig + np.outer(vb, vb)
    grad = None
    if dK is not None:
        u = Q @ v
        W = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - 0.5 * Q @ M @ Q
        grad = np.array([(W * d).sum() for d in dK])
    return mu, sigma, logp, grad


def reference(D, simil, log_theta, X, y, start, events=None, axis=0):
    """The dense closed form at exp(log_theta): (mu, sigma, logp, grad)."""
    K, dK = LR.gram(D, simil, log_theta, X, events, axis, want_grad=True)
    return closed_form(K, y, start, dK)
