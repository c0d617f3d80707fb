"""A numpy restatement of the events case study (tutorial/events), the reference of tests/test_events_*.py.

The descriptor-based oracle cannot express event discounts, so the reference here is written directly from the Go
sources: the discount walk of tutorial/events/kernel/kernel.go:33-44 (swap, first event in list order, break),
Matern52 with the reference's d^2 coefficient 1 (kernel/kernel.go:89-92), a dense K and its Cholesky factor, the LML
of gp/gp.go:244-253, the gradient 1/2 tr((alpha alpha^T - K^-1) dK_p) theta_p of gp/gp.go:418-499 and Produce of
gp/gp.go:258-360 (sigma not clamped).  Kernel: c * Matern52(l) * discount, noise scale * sigma^2 on the diagonal
(tutorial/events/main.go:65-72 with scale 0.01); theta = [c, l | sigma].
"""
import math

import numpy as np

S5 = math.sqrt(5.0)


def discount_pair(events, xa, xb):
    """tutorial/events/kernel/kernel.go:33-44 for one pair, as written there."""
    if xa > xb:
        xa, xb = xb, xa
    for frm, to, disc in events:
        if (xa < frm and frm <= xb) or (xa < to and to <= xb):
            return disc
    return 1.0


def discount_matrix(events, a, b):
    """The same walk for every pair of a (m,) x b (n,): event by event, each pair takes the discount of the first
    event that applies to it (the `break`)."""
    lo = np.minimum(a[:, None], b[None, :])
    hi = np.maximum(a[:, None], b[None, :])
    d = np.ones_like(lo)
    done = np.zeros(lo.shape, dtype=bool)
    for frm, to, disc in events:
        hit = ~done & (((lo < frm) & (frm <= hi)) | ((lo < to) & (to <= hi)))
        d[hit] = disc
        done |= hit
    return d


def _r(A, B, l):
    diff = (A[:, None, :] - B[None, :, :]) / l
    return np.sqrt((diff * diff).sum(-1))


def simil_parts(theta_s, A, B, events, axis):
    """(k, dk/dlog c, dk/dlog l) for every pair of rows of A, B."""
    c, l = theta_s
    r = _r(A, B, l)
    e = np.exp(-S5 * r)
    f = (1.0 + S5 * r + r * r) * e
    dfdlogl = r * r * (3.0 + S5 * r) * e  # df/dr = -r (3 + s5 r) e, dr/dlog l = -r
    d = discount_matrix(events, A[:, axis], B[:, axis]) if events else np.ones_like(r)
    k = c * f * d
    return k, k, c * dfdlogl * d


class RefGP:
    """Dense numpy GP with the events kernel; GP's field / method shape (Observe, Gradient, Produce, X, Y)."""

    def __init__(self, ndim, events, axis=0, noise_scale=0.01):
        self.NDim = ndim
        self.events = [tuple(e) for e in events]
        self.axis = axis
        self.noise_scale = noise_scale
        self.X = np.zeros((0, ndim))
        self.Y = np.zeros(0)
        self.Parallel = False

    def Observe(self, x):
        x = np.asarray(x, dtype=float)
        if x.size > 3:  # gp/gp.go:391-396: inputs and outputs in x
            n = (x.size - 3) // (self.NDim + 1)
            self.X = x[3:3 + n * self.NDim].reshape(n, self.NDim).copy()
            self.Y = x[3 + n * self.NDim:].copy()
        th = np.exp(x[:3])
        self.theta = th
        X, y = np.asarray(self.X, float).reshape(-1, self.NDim), np.asarray(self.Y, float)
        n = len(y)
        K, dc, dl = simil_parts(th[:2], X, X, self.events, self.axis)
        nv = self.noise_scale * th[2] ** 2
        K = K + nv * np.eye(n)
        L = np.linalg.cholesky(K)
        alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
        Kinv = np.linalg.inv(K)
        W = np.outer(alpha, alpha) - Kinv
        self.L, self.alpha, self.K = L, alpha, K
        self.grad = np.array([0.5 * (W * dc).sum(), 0.5 * (W * dl).sum(), 0.5 * np.trace(W) * 2.0 * nv])
        return -0.5 * y @ alpha - np.log(np.diag(L)).sum() - 0.5 * n * math.log(2 * math.pi)

    def Gradient(self):
        return self.grad.copy()

    def Produce(self, Z):
        Z = np.asarray(Z, float).reshape(-1, self.NDim)
        X = np.asarray(self.X, float).reshape(-1, self.NDim)
        prior, _, _ = simil_parts(self.theta[:2], Z, Z, self.events, self.axis)
        var = np.diag(prior).copy()
        if len(X) == 0:
            return np.zeros(len(Z)), np.sqrt(var)
        Ks, _, _ = simil_parts(self.theta[:2], X, Z, self.events, self.axis)
        mu = Ks.T @ self.alpha
        v = np.linalg.solve(self.L, Ks)
        return mu, np.sqrt(var - (v * v).sum(0))


SELFCHECK = "1.0:1.0:0.5,4.2:6.7:0.25"  # tutorial/events/Makefile
