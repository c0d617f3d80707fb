"""kmm32_kernel (cg_mixed.hip: the product with the similarity evaluated in single precision) in isolation, through
launch_kmm32 via the hook gogp_test_kmm32 (run with -m gpu): the inputs, sentinels and shapes of tests/test_cg_kernels.py.

- exact mode (inv_len = 0: f~ = 1 exactly): the output and every slab partial are the integer product bit for bit, for the
  generic instance (two terms) and the fast one (one Normal term, D = 3 padded to 4);
- symmetry: with unit vectors for V the leading block of the output is K~, which equals its transpose bit for bit;
- long double: |got - ref| <= kappa 2^-24 sum_j (sum_t c_t) |V_tj| + the fp64 product's own bound, element by element.
  kappa per family is four times the worst ratio measured on an MI355X (tests/golden/cg_mixed.json), rounded up to a power
  of two, and never above 256: a dropped dimension, a wrong constant or a wrong length is off by 1e-3, far beyond it.
Every launch runs twice and must return the same bits."""
import json
import os

import numpy as np
import pytest

import cg_ref as C
import gram_ref as R
from test_cg_kernels import EXACT_SHAPES, LD_CASES, kmm_inputs, same_bits, sentinels, twice, untouched

pytestmark = pytest.mark.gpu

F64, LD = np.float64, np.longdouble
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cg_mixed.json")))
KAPPA_CAP = 256.0
MIXED_CASES = LD_CASES + [("ard", 8, 0, 0), ("ard", 16, 0, 0)]


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def kappa(family):
    return min(KAPPA_CAP, 2.0 ** np.ceil(np.log2(4.0 * GOLDEN["kappa"][family])))


@pytest.mark.parametrize("rows,cols,T,square", EXACT_SHAPES, ids=["%dx%d-T%d%s" % (s[0], s[1], s[2], "-sq" if s[3] else "")
                                                                  for s in EXACT_SHAPES])
@pytest.mark.parametrize("nslab", [1, 3, 8])
@pytest.mark.parametrize("which", ["generic", "radial1"])
def test_kmm32_exact(gpm, which, rows, cols, T, square, nslab):
    D = 3
    kp = R.exact_kp(which, D)
    csum = sum(t["c"] for t in kp.terms)
    A, B, V, ldv, diag = kmm_inputs(D, rows, cols, T, square, True)
    centre = np.concatenate([np.array([0.25, -0.5, 0.0]), sentinels(1)])
    rpad, ldo = -(-rows // 64) * 64, rows + 5
    Vm = V.reshape(T + 1, ldv)[:T, :cols]
    for max_blocks in (0, 2):
        part0, out0 = sentinels(nslab * T * rpad + 7), sentinels(T * ldo + 7)
        part, out = twice(lambda: gpm.kmm32_check(kp.hook(gpm), A, rows, B, cols, centre, V, ldv, T, diag, nslab, part0, out0,
                                                  ldo, max_blocks=max_blocks))
        want = csum * Vm.sum(axis=1)[:, None] * np.ones((T, rows))
        if square:
            want = want + Vm * diag[None, :]
        body = out[:T * ldo].reshape(T, ldo)
        assert same_bits(body[:, :rows], want), "output"
        assert same_bits(body[:, rows:], np.zeros((T, ldo - rows))), "the padded rows of the output are zero"
        assert untouched(out[T * ldo:]) and untouched(part[nslab * T * rpad:])
        pm = part[:nslab * T * rpad].reshape(nslab, T, rpad)
        for s, (a, b) in enumerate(C.slab_columns(cols, nslab)):
            ws = csum * Vm[:, a:b].sum(axis=1)[:, None] * np.ones((T, rows))
            if square:
                ws[:, a:b] += Vm[:, a:b] * diag[None, a:b]
            assert same_bits(pm[s][:, :rows], ws), "partials of slab %d" % s
            assert same_bits(pm[s][:, rows:], np.zeros((T, rpad - rows))), "padded rows of slab %d" % s


@pytest.mark.parametrize("case", [("matern52", 8, 0, 0), ("max_terms", 3, 0, 0), ("periodic", 3, 0, 0)], ids=R.case_id)
def test_kmm32_symmetric(gpm, case):
    kp, D, n, T = R.kp_of(case), case[1], 80, 64
    A = np.random.default_rng([95, D]).uniform(-1.0, 1.0, n * D)
    V = np.eye(T, n).reshape(-1)
    nslab, rpad = 2, 128
    _, out = twice(lambda: gpm.kmm32_check(kp.hook(gpm), A, n, None, n, np.zeros(D), V, n, T, None, nslab,
                                           sentinels(nslab * T * rpad), sentinels(T * n), n))
    K = out.reshape(T, n)[:, :T]
    assert np.isfinite(K).all() and K.min() > 0 and same_bits(K, K.T.copy())


@pytest.mark.parametrize("case", MIXED_CASES, ids=[R.case_id(c) for c in MIXED_CASES])
def test_kmm32_long_double(gpm, case):
    kp, D, n = R.kp_of(case), case[1], 193
    csum = sum(abs(t["c"]) for t in kp.terms)
    worst = 0.0
    for T in (1, 17, 64):
        square = T == 17
        rows, cols = (n, n) if square else (n, 130)
        A, B, V, ldv, diag = kmm_inputs(D, rows, cols, T, square, False, seed=1)
        a = A[:rows * D].reshape(rows, D)
        b = a if square else B[:cols * D].reshape(cols, D)
        pts = np.concatenate([a, b])
        centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
        nslab, rpad, ldo = 3, -(-rows // 64) * 64, rows + 1
        part0, out0 = sentinels(nslab * T * rpad), sentinels(T * ldo)
        _, out = twice(lambda: gpm.kmm32_check(kp.hook(gpm), A, rows, B, cols, centre, V, ldv, T, diag, nslab, part0, out0, ldo))
        Vm = V.reshape(T + 1, ldv)[:T, :cols]
        want, bound = C.kmm(kp, a, b, Vm, diag)
        got = out.reshape(T, ldo)
        assert np.isfinite(got).all() and same_bits(got[:, rows:], np.zeros((T, ldo - rows)))
        err = np.abs(got[:, :rows].astype(LD) - want).astype(F64)
        unit = 2.0 ** -24 * csum * np.abs(Vm).sum(axis=1)[:, None]
        worst = max(worst, float((np.maximum(err - bound, 0.0) / unit).max()))
    print("kmm32 %s: worst (|err| - fp64 bound) / (2^-24 sum c |V|) = %.3g (kappa %g)" % (R.case_id(case), worst, kappa(case[0])))
    assert kappa(case[0]) <= KAPPA_CAP and worst <= kappa(case[0])
