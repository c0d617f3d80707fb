"""Per-observation noise variances (gogp_set_noise_variances): the inputs its tests share and the dense numpy fp64
reference, on top of the oracle's gram_np.

    K     = k(X, X) + s2(theta) I + diag(v) = L L^T,  alpha = K^-1 y,  W = alpha alpha^T - K^-1
    LML   = -n/2 log 2 pi - sum_i log L_ii - 1/2 y^T alpha
    dLML / d log theta_p = 1/2 sum_ab W_ab dK_ab / d log theta_p   (UniformNoise: dK / d log theta_n = 2 s2 I; diag(v) has
                                                                    no derivative in theta)
    dLML / dv_i = 1/2 W_ii
    Produce: mu = Ks^T alpha, sigma^2 = k(z, z) - diag(Ks^T K^-1 Ks) (no noise term), the joint covariance likewise
    LOO:  tests/loo_ref.py closed_form on this K (sigma_i then includes v_i)
    HeteroscedasticModel: v = exp(G phi), d / dphi = G^T (v o dv)

Inputs: noise std 0.1 (s2 = 0.01), v log-normal over roughly [0, 4 s2] with several entries exactly 0, X uniform in
[-2, 2]^D: cond(K) stays below 1e5 on every case the GPU tests use (tests/test_noise_variances_cpu.py checks it), where the
reference alone sits far inside the suite's tolerances.
"""
import numpy as np

import events_ref as R
from gogp_amd import kernel
from oracle.oracle import gram_np
from produce_grad_ref import EVENTS, FAMILIES, FOUR  # noqa: F401  (shared with the tests)

NOISE = kernel.UniformNoise
TN = [0.1]  # noise variance 0.01
S2 = TN[0] ** 2
MAIN = "matern32_2d"
LOG_2PI = float(np.log(2.0 * np.pi))

#: the sizes of the GPU tests: 1, 2, 20 and 128 would take the one-launch form without variances, 129 is the first ragged
#: size, 700 has npad = 768 so that the diagonal crosses the 512-column boundary between the two streams' parts
SHAPES = [1, 2, 20, 128, 129, 300, 700, 1100]
PRODUCE_M = [1, 64, 200]
COND_MAX = 1e5


def inputs(n, D, m=200, seed=11):
    """X uniform in [-2, 2]^D, y = sin(sum x) + noise of the variances below, Z uniform in [-2.5, 2.5]^D."""
    rng = np.random.default_rng(seed + 1000 * D + n)
    X = rng.uniform(-2.0, 2.0, (n, D))
    v = variances(n, seed)
    y = np.sin(X.sum(1)) + np.sqrt(S2 + v) * rng.normal(size=n)
    Z = rng.uniform(-2.5, 2.5, (m, D))
    return X, y, v, Z


def variances(n, seed=11):
    """Log-normal around s2, capped at 4 s2; every fifth entry from the second on exactly 0."""
    rng = np.random.default_rng(seed + 77 + n)
    v = np.minimum(S2 * np.exp(rng.normal(-0.3, 0.9, size=n)), 4.0 * S2)
    v[1::5] = 0.0
    return v


def log_theta(fam):
    return np.log(list(FAMILIES[fam][2]) + TN)


class Ref:
    """The dense GP with K = k + s2 I + diag(v); `simil` without its events, which are given apart."""

    def __init__(self, D, simil, X, y, v=None, noise=NOISE, events=None, axis=0):
        self.D, self.simil, self.noise = D, simil, noise
        self.desc = kernel.build_desc(D, simil, noise)
        self.ns = self.desc.ntheta_simil
        self.nn = 0 if self.desc.noise_kind == kernel.NOISE_CONSTANT else 1
        self.X = np.asarray(X, float).reshape(-1, D)
        self.y = np.asarray(y, float).reshape(-1)
        self.v = np.zeros(len(self.y)) if v is None else np.asarray(v, float).reshape(-1)
        self.events, self.axis = events, axis

    def noise_var(self, tn):
        if self.desc.noise_kind in (kernel.NOISE_CONSTANT, kernel.NOISE_CONSTANT_PARAM):
            return self.desc.noise_std ** 2
        return self.desc.noise_scale * tn[0] ** 2

    def _cross(self, A, B):
        K = gram_np(self.desc, self.ts, A, B)
        if self.events:
            K = K * R.discount_matrix(self.events, A[:, self.axis], B[:, self.axis])
        return K

    def gram(self, x, want_grad=False):
        """K at theta = exp(x) and, want_grad, the list of dK / d log theta_p (the noise parameter last, if any)."""
        th = np.exp(np.asarray(x, float).reshape(-1))
        self.ts, self.tn = th[:self.ns], th[self.ns:]
        n = len(self.y)
        out = gram_np(self.desc, self.ts, self.X, self.X, want_grad=want_grad)
        K, dK = out if want_grad else (out, None)
        if self.events:
            Dm = R.discount_matrix(self.events, self.X[:, self.axis], self.X[:, self.axis])
            K = K * Dm
            dK = [d * Dm for d in dK] if want_grad else None
        s2 = self.noise_var(self.tn)
        K = K + s2 * np.eye(n) + np.diag(self.v)
        if not want_grad:
            return K
        dK = list(dK)
        if self.nn:
            uniform = self.desc.noise_kind == kernel.NOISE_UNIFORM
            dK.append((2.0 * s2 if uniform else 0.0) * np.eye(n))
        return K, dK

    def lml_only(self, x, v=None):
        """The LML at exp(x) and the variances v (default: the object's), nothing stored: for finite differences."""
        keep = self.v
        if v is not None:
            self.v = np.asarray(v, float)
        K = self.gram(x)
        self.v = keep
        L = np.linalg.cholesky(K)
        a = np.linalg.solve(L.T, np.linalg.solve(L, self.y))
        return -0.5 * len(self.y) * LOG_2PI - np.log(np.diag(L)).sum() - 0.5 * float(self.y @ a)

    def observe(self, x):
        self.K, self.dK = self.gram(x, want_grad=True)
        n = len(self.y)
        self.L = np.linalg.cholesky(self.K)
        self.alpha = np.linalg.solve(self.L.T, np.linalg.solve(self.L, self.y))
        Li = np.linalg.solve(self.L, np.eye(n))
        self.Kinv = Li.T @ Li
        self.lml = -0.5 * n * LOG_2PI - np.log(np.diag(self.L)).sum() - 0.5 * float(self.y @ self.alpha)
        self.W = np.outer(self.alpha, self.alpha) - self.Kinv
        self.grad = np.array([0.5 * float((self.W * d).sum()) for d in self.dK])
        self.dv = 0.5 * np.diag(self.W).copy()
        return self.lml

    def produce(self, Z, cov=False):
        Z = np.asarray(Z, float).reshape(-1, self.D)
        Ks = self._cross(self.X, Z)
        V = np.linalg.solve(self.L, Ks)
        mu = Ks.T @ self.alpha
        if cov:
            return mu, self._cross(Z, Z) - V.T @ V
        prior = np.array([gram_np(self.desc, self.ts, Z[i:i + 1], Z[i:i + 1])[0, 0] for i in range(len(Z))])
        return mu, np.sqrt(prior - (V * V).sum(0))

    def hetero(self, x, G):
        """(LML, gradient) of HeteroscedasticModel at x = [log theta | phi]: v = exp(G phi)."""
        P = self.ns + self.nn
        x = np.asarray(x, float).reshape(-1)
        G = np.asarray(G, float)
        self.v = np.exp(G @ x[P:])
        lml = self.observe(x[:P])
        return lml, np.concatenate([self.grad, G.T @ (self.v * self.dv)])


def assert_lml(got, want, tag=""):
    assert abs(got - want) <= 1e-8 * abs(want), (tag, got, want)


def assert_vector(got, want, tag=""):
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8, err_msg=str(tag))


def assert_gradient(got, want, tag=""):
    """Every component within 1e-6 of the largest absolute component (the suite's rule for gradients; dv too)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if want.size == 0:
        return
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max |err| = %.3e of largest component %.3e" % (tag, err, scale))
    assert err <= 1e-6 * scale, (tag, err, scale)
