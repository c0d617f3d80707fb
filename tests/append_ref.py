"""gogp_append (GP.Append): the inputs its tests share and a numpy restatement of the block update.

With K = [K11 B^T; B C] and K11 = L11 L11^T, rows join the factor in chunks of at most 64:
    L21 = B L11^-T,  S = C - L21 L21^T,  L22 = chol(S),  z2 = L22^-1 (y2 - L21 z1),  alpha = L^-T z,
    LML = -(n + m)/2 log 2 pi - sum log L_ii - 1/2 y^T alpha.
"""
import math

import numpy as np

from gogp_amd import kernel, synth

CHUNK = 64

#: name -> (NDim, Simil, Noise, theta_simil, theta_noise); theta as tests/cases.py, noise std >= 0.1
FAMILIES = {
    "scaled_rbf3": (3, kernel.Scaled(kernel.Normal), kernel.UniformNoise, [1.0, 0.8], [0.1]),
    "matern32": (1, kernel.Scaled(kernel.Matern32), kernel.UniformNoise, [1.0, 0.7], [0.15]),
    "hyperpriors": (1, kernel.Sum([kernel.Scaled(kernel.Matern52),
                                   kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))], order=[0, 2, 1, 3, 4]),
                    kernel.ScaledNoise(0.01), [1.0, 0.5, 0.6, 1.3, 0.05], [2.0]),
    "ard_rbf3": (3, kernel.Scaled(kernel.ARD(kernel.Normal, 3)), kernel.UniformNoise, [1.2, 0.9, 1.0, 1.1], [0.2]),
}

#: (n, m, family): the smallest shapes at which each mechanism of the update can go wrong
SHAPES = [
    (0, 5, "scaled_rbf3"),      # empty process: append = absorb
    (1, 1, "matern32"),         # single row
    (100, 1, "hyperpriors"),    # stays inside the one-launch range (N <= 128)
    (127, 2, "ard_rbf3"),       # leaves it
    (250, 6, "scaled_rbf3"),    # fills a 256-block exactly, npad unchanged
    (250, 7, "matern32"),       # crosses into a new 256-block: restride, new block inverse, new padding
    (256, 1, "hyperpriors"),    # starts a new 256-block
    (300, 64, "ard_rbf3"),      # a full chunk
    (300, 65, "scaled_rbf3"),   # two chunks, the block inverse refreshed between them
    (200, 330, "matern32"),     # more new rows than a block, three npad values in one call
]
RESTORED = (600, 40, "scaled_rbf3")   # after restore(L, Alpha): no z on the handle
REPEATED = (200, 120, "hyperpriors")  # one row at a time, crossing 256 once
M_TEST = 7


def inputs(n_total, D, seed=11):
    X, y = synth.make_inputs(n_total, D, seed)
    return X, y, synth.make_test_points(M_TEST, D, seed)


def shape_id(s):
    return "%d+%d-%s" % s


def block_append(K, y, n, chunk=CHUNK):
    """(L, alpha, lml) of the whole K by the block update from the factor of K[:n, :n]."""
    N = len(y)
    L = np.zeros((N, N))
    z = np.zeros(N)
    if n > 0:
        L[:n, :n] = np.linalg.cholesky(K[:n, :n])
        z[:n] = np.linalg.solve(L[:n, :n], y[:n])
    cur = n
    while cur < N:
        e = min(N, cur + chunk)
        if cur > 0:
            L21 = np.linalg.solve(L[:cur, :cur], K[cur:e, :cur].T).T
        else:
            L21 = np.zeros((e - cur, 0))
        S = K[cur:e, cur:e] - L21 @ L21.T
        L22 = np.linalg.cholesky(S)
        L[cur:e, :cur] = L21
        L[cur:e, cur:e] = L22
        z[cur:e] = np.linalg.solve(L22, y[cur:e] - L21 @ z[:cur])
        cur = e
    alpha = np.linalg.solve(L.T, z)
    lml = -0.5 * N * math.log(2 * math.pi) - np.log(np.diag(L)).sum() - 0.5 * y @ alpha
    return L, alpha, lml


def assert_state(lml, alpha, L, lml_o, alpha_o, L_o, tag=""):
    """The tolerances of tests/test_gpu_parity.py::_check_against."""
    assert abs(lml - lml_o) <= 1e-8 * max(1.0, abs(lml_o)), (tag, lml, lml_o)
    np.testing.assert_allclose(alpha, alpha_o, rtol=1e-6, atol=1e-8 * np.abs(alpha_o).max(), err_msg=str(tag))
    np.testing.assert_allclose(L, L_o, rtol=1e-8, atol=1e-10, err_msg=str(tag))


def assert_produce(mu, sigma, mu_o, sigma_o, tag=""):
    np.testing.assert_allclose(mu, mu_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
    np.testing.assert_allclose(sigma, sigma_o, rtol=1e-6, atol=1e-8, err_msg=str(tag))
