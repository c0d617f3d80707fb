"""The two kernels of csrc/pathwise.hip alone, through their test hooks, against long doubles (run with -m gpu).  Shapes:
ragged against every tile edge (16 features, 4 dimensions, 16 samples, 64 points), more than one workgroup, and (130
points, 130 features) more than one slab of features."""
import numpy as np
import pytest

import pathwise_ref as PR
from gogp_amd import kernel, pathwise
from gogp_amd.gp import kparams

pytestmark = pytest.mark.gpu
LD, EPS = PR.LD, PR.EPS

#: name -> terms at NDim dimensions (pathwise_ref.kern)
KERNELS = {
    "normal": lambda D: [dict(kind=kernel.K_NORMAL, c=1.3, il=np.full(D, 1 / 0.7))],
    "matern32": lambda D: [dict(kind=kernel.K_MATERN32, c=0.8, il=np.full(D, 1 / 0.9))],
    "ard_sum": lambda D: [dict(kind=kernel.K_NORMAL, c=0.6, il=1 / np.linspace(0.5, 1.1, D), ard=True),
                          dict(kind=kernel.K_MATERN52_TEXTBOOK, c=1.1, il=np.full(D, 1 / 1.4))],
}


def features(points, D, R, S, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, D)) / np.sqrt(D), rng.uniform(0, 2 * np.pi, R), rng.uniform(0.1, 1.0, R),
            rng.uniform(-1, 1, (points, D)), rng.standard_normal((R, S)))


@pytest.mark.parametrize("points, D, R, S", [(1, 1, 5, 1), (65, 3, 17, 17), (130, 8, 130, 64)])
def test_feature_product_value_and_gradient(points, D, R, S):
    Omega, phase, amp, Z, W = features(points, D, R, S)
    aw = (np.abs(amp)[:, None] * np.abs(W)).sum(0).max()
    bound = (R + 8) * EPS * aw + EPS * np.abs(phase).max() * aw
    F = pathwise.features_check(Omega, phase, amp, Z, W)
    Fref = (PR.feats(Omega, phase, amp, Z) @ W.astype(LD)).T
    dF = pathwise.features_check(Omega, phase, amp, Z, W, grad=True)
    dref = np.einsum("ird,rs->sid", PR.feats(Omega, phase, amp, Z, deriv=True), W.astype(LD))
    ev, eg = float(np.abs(F - Fref).max()), float(np.abs(dF - dref).max())
    print("features %s: error / bound: value %.3f, gradient %.3f" % ((points, D, R, S), ev / bound,
                                                                     eg / (bound * np.abs(Omega).max())))
    assert ev <= bound and eg <= bound * np.abs(Omega).max()


@pytest.mark.parametrize("m, n, D, S", [(1, 37, 1, 1), (65, 129, 3, 17)])
@pytest.mark.parametrize("name", list(KERNELS))
def test_cross_gradient(name, m, n, D, S):
    rng = np.random.default_rng(5)
    terms = KERNELS[name](D)
    X, Z, V = rng.uniform(0, 3, (n, D)), rng.uniform(0, 3, (m, D)), rng.standard_normal((S, n))
    Z[0] = X[3]  # a coincident pair: its derivative is 0, also where r = 0 is a kink of the formula (Matern-3/2)
    kp = kparams(D, [dict(kind=t["kind"], c=t["c"], inv_len=t["il"], ard=t.get("ard", False)) for t in terms])
    G = pathwise.crossgrad_check(kp, Z, X, V)
    dk = PR.kern(terms, Z, X, deriv=True)
    Gref = np.einsum("ijd,sj->sid", dk, V.astype(LD))
    bound = n * EPS * float(np.abs(dk).max()) * np.abs(V).sum(1).max() / n * 16
    err = float(np.abs(G - Gref).max())
    print("crossgrad %s %s: error / bound %.3f" % (name, (m, n, D, S), err / bound))
    assert np.all(dk[0, 3] == 0) and err <= bound


def test_a_column_has_the_same_bits_alone_as_among_seventeen():
    Omega, phase, amp, Z, W = features(65, 3, 17, 17)
    for grad in (False, True):
        assert np.array_equal(pathwise.features_check(Omega, phase, amp, Z, W, grad)[4],
                              pathwise.features_check(Omega, phase, amp, Z, W[:, 4:5], grad)[0])
    rng = np.random.default_rng(6)
    X, V = rng.uniform(0, 3, (129, 3)), rng.standard_normal((17, 129))
    kp = kparams(3, [dict(kind=kernel.K_MATERN32, c=0.8, inv_len=1 / 0.9)])
    assert np.array_equal(pathwise.crossgrad_check(kp, Z, X, V)[4], pathwise.crossgrad_check(kp, Z, X, V[4:5])[0])
