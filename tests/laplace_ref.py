"""Non-Gaussian likelihoods by the Laplace approximation (gogp_laplace_*): the numpy restatement its tests share.
Families, events, noise and inputs: those of tests/loo_ref.py.

With K = k(X, X) + theta_n^2 I (the noise is the latent nugget), pi = 1 / (1 + exp(-f)) and per observation
    bernoulli:  log p = y f - softplus(f),             g = y - pi,      W = pi (1 - pi),  rho = 2 pi - 1
    poisson:    log p = y f - exp(f) - lgamma(y + 1),  g = y - exp(f),  W = exp(f),       rho = -1
the mode is found by Rasmussen & Williams' Algorithm 3.1 in a = K^-1 f, damped:
    sw = sqrt(W), b = W f + g, B = I + diag(sw) K diag(sw) = L L^T, a+ = b - sw o B^-1 (sw o (K b)),
    a <- a + t (a+ - a), t = 1, 1/2, ... while psi(a) = -1/2 a^T f + sum log p drops by more than the rounding of its
    sums (1e-12 max(1, |psi|)); 20 halvings at the most;
    converged when |a - g(f)|_inf <= tol max(1, |a|_inf); B is factored AT the returned iterate;
    Z = psi - sum log L_ii.
Gradient (B^-1 explicit, R = diag(sw) B^-1 diag(sw)):
    s_i = +1/2 (1 - [B^-1]_ii) rho_i,  u = s - R (K s),  G = R - u a^T - a u^T,
    dZ / d log theta_p = 1/2 sum_ab (a a^T - G)_ab dK_ab / d log theta_p.
R&W eq. 5.23 and the s2 line of Alg. 5.1 have the opposite sign of s (``sign=-1`` here): tests/test_laplace_cpu.py
shows that a central difference of Z refuses it.
Prediction: mu = k*^T a, sigma^2 = k(z, z) - |L^-1 (sw o k*)|^2; poisson mean exp(mu + sigma^2 / 2), bernoulli mean
int pi(f) N(f | mu, sigma^2) df by the 32-point Gauss-Hermite rule.
"""
import math

import numpy as np

import events_ref as R
from gogp_amd import kernel
from loo_ref import EVENTS, FAMILIES, NOISE, TN, gram, inputs  # noqa: F401  (shared with the tests)
from oracle.oracle import gram_np

BERNOULLI, POISSON = 0, 1
_LGAMMA = np.vectorize(math.lgamma)
GH_X, GH_W = np.polynomial.hermite.hermgauss(32)


def logistic(f):
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sites(lik, f, y):
    """(log p, g, W, rho) per observation, in forms that do not overflow for |f| ~ 700"""
    f, y = np.asarray(f, float), np.asarray(y, float)
    if lik == BERNOULLI:
        e = np.exp(-np.abs(f))
        d = 1.0 / (1.0 + e)
        pi = np.where(f >= 0, d, e * d)
        return y * f - (np.maximum(f, 0.0) + np.log1p(e)), y - pi, e * d * d, 2.0 * pi - 1.0
    ef = np.exp(f)
    return y * f - ef - _LGAMMA(y + 1.0), y - ef, ef, -np.ones_like(f)


def valid(lik, y):
    y = np.asarray(y, float)
    if lik == BERNOULLI:
        return bool(np.all((y == 0) | (y == 1)))
    return bool(np.all((y >= 0) & (y == np.floor(y)) & np.isfinite(y)))


def draw(lik, K, seed=3):
    """y drawn once, with a fixed seed, from the model itself: f = L xi with K = L L^T; poisson rate exp(f + 1) (prior
    variances <= 2.3 keep the counts at a few tens), bernoulli P(y = 1) = logistic(f)."""
    rng = np.random.default_rng(seed + len(K))
    f = np.linalg.cholesky(K) @ rng.normal(size=len(K))
    if lik == BERNOULLI:
        return (rng.uniform(size=len(K)) < logistic(f)).astype(float)
    return rng.poisson(np.exp(f + 1.0)).astype(float)


class Fit:
    """The result of mode(): a, f, the site vectors at them, the Cholesky factor of B, Z, the steps taken."""


def mode(lik, K, y, tol=1e-10, max_iter=50, a0=None, strict=False):
    """strict: a step must INCREASE psi (no slack for the rounding of its sums): what the slack is there to avoid"""
    y = np.asarray(y, float)
    n = len(y)
    a = np.zeros(n) if a0 is None else np.array(a0, float)
    f = K @ a
    lp, g, W, rho = sites(lik, f, y)
    psi = -0.5 * (a @ f) + lp.sum()
    its, stuck = 0, False
    while True:
        conv = (not stuck) and np.abs(a - g).max(initial=0.0) <= tol * max(1.0, np.abs(a).max(initial=0.0))
        sw = np.sqrt(W)
        B = np.eye(n) + sw[:, None] * K * sw[None, :]
        L = np.linalg.cholesky(B)
        if conv or stuck or its >= max_iter:
            break
        b = W * f + g
        beta = np.linalg.solve(L.T, np.linalg.solve(L, sw * (K @ b)))
        a1 = b - sw * beta
        f1 = K @ a1
        t, halvings = 1.0, 0
        while True:
            at, ft = a + t * (a1 - a), f + t * (f1 - f)
            lpt, gt, Wt, rhot = sites(lik, ft, y)
            psit = -0.5 * (at @ ft) + lpt.sum()
            if (psit > psi) if strict else (psit >= psi - 1e-12 * max(1.0, abs(psi))):
                break
            halvings += 1
            if halvings > 20:
                stuck = True
                break
            t *= 0.5
        if stuck:
            continue
        a, f, lp, g, W, rho, psi = at, ft, lpt, gt, Wt, rhot, psit
        its += 1
    r = Fit()
    r.a, r.f, r.g, r.W, r.sw, r.rho, r.L, r.B = a, f, g, W, sw, rho, L, B
    r.psi, r.Z = psi, psi - np.log(np.diag(L)).sum()
    r.iterations, r.converged = its, bool(conv)
    return r


def gradient(fit, K, dK, sign=+1.0):
    """dZ / d log theta from the list dK of derivative matrices; sign = -1: the sign of s as printed in R&W"""
    Binv = np.linalg.inv(fit.B)
    Binv = 0.5 * (Binv + Binv.T)
    sw, a = fit.sw, fit.a
    Rm = sw[:, None] * Binv * sw[None, :]
    s = sign * 0.5 * (1.0 - np.diag(Binv)) * fit.rho
    u = s - Rm @ (K @ s)
    G = Rm - np.outer(u, a) - np.outer(a, u)
    Wm = np.outer(a, a) - G
    return np.array([0.5 * (Wm * d).sum() for d in dK])


def gh_mean(lik, mu, sigma, points=32):
    mu, sigma = np.asarray(mu, float), np.asarray(sigma, float)
    if lik == POISSON:
        return np.exp(mu + 0.5 * sigma * sigma)
    x, w = (GH_X, GH_W) if points == 32 else np.polynomial.hermite.hermgauss(points)
    return (w[None, :] * logistic(mu[:, None] + math.sqrt(2.0) * sigma[:, None] * x[None, :])).sum(1) / math.sqrt(math.pi)


def predict(lik, fit, Ks, prior):
    """(mu, sigma, mean) from Ks = k(X, Z) (n x m, no noise) and prior = k(z, z)"""
    mu = Ks.T @ fit.a
    V = np.linalg.solve(fit.L, fit.sw[:, None] * Ks)
    sigma = np.sqrt(prior - (V * V).sum(0))
    return mu, sigma, gh_mean(lik, mu, sigma)


def cross(D, simil, log_theta, X, Z, events=None, axis=0):
    """(k(X, Z), k(z, z)) at theta = exp(log_theta), discounts applied"""
    desc = kernel.build_desc(D, simil, NOISE)
    ths = np.exp(np.asarray(log_theta, float))[:-1]
    X, Z = np.asarray(X, float).reshape(-1, D), np.asarray(Z, float).reshape(-1, D)
    prior = np.diag(gram_np(desc, ths, Z, Z)).copy()
    if len(X) == 0:
        return np.zeros((0, len(Z))), prior
    Ks = gram_np(desc, ths, X, Z)
    if events:
        Ks = Ks * R.discount_matrix(events, Z[:, axis], X[:, axis]).T
    return Ks, prior


def reference(lik, D, simil, log_theta, X, y, events=None, axis=0, **kw):
    """(fit, gradient) of the dense reference at exp(log_theta)"""
    K, dK = gram(D, simil, log_theta, X, events, axis, want_grad=True)
    fit = mode(lik, K, y, **kw)
    return fit, gradient(fit, K, dK)
