"""The kernels of the Laplace approximation (gogp_amd/csrc/laplace.hip) in isolation, through their test hooks, against
numpy at n = 1, 63, 64, 65, 129, 300: the ragged edges of the 64-tiles and the first two-panel size (npad = 256 or 512).

Exact parts are held to the bit:
  * products of two or three float64 numbers in the kernel's order (IEEE multiplication is correctly rounded on both
    sides): the scaled Gram matrix, the column scaling, sw o beta, s from the diagonal;
  * a f, |a - g| and |a| from the kernel's own g, and their block sums and maxima in the kernel's order -- 64 lanes by
    a butterfly, four waves as (w0 + w1) + (w2 + w3), the blocks in block order;
  * every expression with a sum behind a product (the compiler may fuse them) on small dyadic operands, where no
    rounding happens at all: a+ = b - sw o beta, the interpolation, u, the weight matrix;
  * the zeros from row n on, the padding of the Gram matrix, everything outside the tiles a kernel owns.
Transcendental parts (exp, log1p, lgamma, sqrt behind them) are held to rtol = 1e-14, about 45 ulp for chains of up to
four library calls at <= 4 ulp each.  Where the last operation subtracts numbers of size S (g = y - pi, rho = 2 pi - 1,
b = W f + g) the result is held to 1e-14 |want| + 4 eps S: its error is absolute in S, not relative in itself.  Sums of
such parts: 1e-14 of the sum of the terms' magnitudes.  Rounded general operands of the fused expressions: 4 eps of
the sum of the terms' magnitudes (dot products of length n: (n + 8) eps).  f includes +-40 and +-700: nothing may
come out as NaN or inf."""
import math

import numpy as np
import pytest

import laplace_ref as LP
from gogp_amd import gp

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 129, 300)
EPS = np.finfo(float).eps
LIKS = [LP.BERNOULLI, LP.POISSON]
IDS = ["bernoulli", "poisson"]


def npad_of(n):
    return (n + 255) // 256 * 256


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, float).view(np.uint64), np.ascontiguousarray(b, float).view(np.uint64))


def dyadic(rng, shape, lo=-8, hi=8):
    """multiples of 1/8 of small size: products and sums of a few of them are exact in float64"""
    return rng.integers(lo * 8, hi * 8 + 1, shape).astype(float) / 8.0


def block_reduce(v, op):
    """The kernel's order over one 256-row block: a butterfly over the 64 lanes of each wave (lane 0's result), then
    (w0 op w1) op (w2 op w3)."""
    w = []
    for k in range(4):
        x = v[64 * k:64 * k + 64].copy()
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            x = op(x, x[idx ^ o])
        w.append(x[0])
    return op(op(w[0], w[1]), op(w[2], w[3]))


def site_inputs(n, lik, seed=0):
    rng = np.random.default_rng(100 * n + lik + seed)
    f = np.concatenate([[700.0, -700.0, 40.0, -40.0, 0.0], 3.0 * rng.normal(size=n)])[:n]
    if n == 1:
        f = np.array([-700.0])
    y = (rng.uniform(size=n) < 0.5).astype(float) if lik == LP.BERNOULLI else rng.poisson(6.0, n).astype(float)
    a = rng.normal(size=n)
    return f, y, a


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
@pytest.mark.parametrize("n", NS)
def test_site_kernel(n, lik):
    npad, nb = npad_of(n), npad_of(n) // 256
    f, y, a = site_inputs(n, lik)
    z = np.full(npad, np.nan)
    g, W, sw, b, rho, part, out = gp.laplace_kernel_check("lap_site", 0, lik=lik, f=f, y=y, a=a, n=n, npad=npad, g=z, W=z,
                                                          sw=z, b=z, rho=z, part=np.full(5 * nb, np.nan), out=np.full(5, np.nan))
    lp_o, g_o, W_o, rho_o = LP.sites(lik, f, y)
    for v in (g, W, sw, b, rho, part, out):
        assert np.all(np.isfinite(v))
    for v in (g, W, sw, b, rho):
        assert not v[n:].any()
    S = np.ones(n) if lik == LP.BERNOULLI else np.maximum(y, np.exp(f))
    err = lambda got, want, s: (np.abs(got - want) / (1e-14 * np.abs(want) + 4 * EPS * s)).max()  # noqa: E731
    b_o = W_o * f + g_o
    figs = (err(g[:n], g_o, S), err(W[:n], W_o, 0 * S), err(sw[:n], np.sqrt(W_o), 0 * S), err(rho[:n], rho_o, S),
            err(b[:n], b_o, np.abs(W_o * f) + np.abs(g_o)))
    print("site n = %d lik = %d: g %.3f W %.3f sw %.3f rho %.3f b %.3f of their bounds" % ((n, lik) + figs))
    assert max(figs) <= 1.0
    assert same_bits(sw[:n], np.sqrt(W[:n]))  # sqrt is correctly rounded
    # the block results in the kernel's order, from the kernel's own g where they depend on it
    pad = lambda v: np.concatenate([v, np.zeros(npad - n)])  # noqa: E731
    af, res, am = pad(a * f), pad(np.abs(a - g[:n])), pad(np.abs(a))
    for k in range(nb):
        blk = slice(256 * k, 256 * k + 256)
        assert part[1 * nb + k] == block_reduce(af[blk], np.add)
        assert part[2 * nb + k] == block_reduce(res[blk], np.maximum)
        assert part[3 * nb + k] == block_reduce(am[blk], np.maximum)
        assert part[4 * nb + k] == -1.0
    tot = 0.0
    for k in range(nb):
        tot += part[1 * nb + k]
    assert out[1] == tot and out[2] == part[2 * nb:3 * nb].max() and out[3] == part[3 * nb:4 * nb].max() and out[4] == -1.0
    lp_terms = np.abs(y * f) + (np.maximum(f, 0) + np.log1p(np.exp(-np.abs(f))) if lik == LP.BERNOULLI
                                else np.exp(f) + np.abs(LP._LGAMMA(y + 1.0)))
    lp_sum = sum(part[0 * nb + k] for k in range(nb))
    assert out[0] == lp_sum
    print("site n = %d lik = %d: sum log p %.15e (numpy %.15e), bound %.3e" % (n, lik, out[0], lp_o.sum(), 1e-14 * lp_terms.sum()))
    assert abs(out[0] - lp_o.sum()) <= 1e-14 * lp_terms.sum()
    if lik == LP.POISSON and n > 1:  # exp(700) swamps that sum: once more at moderate f, where every term counts
        f2 = np.clip(f, -40.0, 4.0)
        out2 = gp.laplace_kernel_check("lap_site", 0, lik=lik, f=f2, y=y, a=a, n=n, npad=npad, g=z, W=z, sw=z, b=z, rho=z,
                                       part=np.full(5 * nb, np.nan), out=np.full(5, np.nan))[-1]
        terms2 = np.abs(y * f2) + np.exp(f2) + np.abs(LP._LGAMMA(y + 1.0))
        want2 = LP.sites(lik, f2, y)[0].sum()
        print("site n = %d lik = %d, |f| moderate: sum log p %.15e (numpy %.15e), bound %.3e"
              % (n, lik, out2[0], want2, 1e-14 * terms2.sum()))
        assert abs(out2[0] - want2) <= 1e-14 * terms2.sum()


@pytest.mark.parametrize("lik", LIKS, ids=IDS)
def test_site_kernel_marks_the_first_refused_y(lik):
    n, npad = 300, 512
    f, y, a = site_inputs(n, lik)
    z = np.zeros(npad)
    for rows in ([299], [70, 260], [257, 258], [0]):
        yy = y.copy()
        yy[rows] = 0.5 if lik == LP.BERNOULLI else -1.0
        out = gp.laplace_kernel_check("lap_site", 0, lik=lik, f=f, y=yy, a=a, n=n, npad=npad, g=z, W=z, sw=z, b=z, rho=z,
                                      part=np.zeros(10), out=np.zeros(5))
        assert out[-1][4] == float(rows[0])
        assert not out[1][rows].any()  # W of a refused row is zero: nothing of it spreads


@pytest.mark.parametrize("wcols", [0, 64, 256])
@pytest.mark.parametrize("n", NS)
def test_scaled_gram(n, wcols):
    npad, ld = npad_of(n), npad_of(n) + 8
    rng = np.random.default_rng(n + wcols)
    A = rng.normal(size=(npad, ld))
    A[n:npad, :] = 0.0
    A[:, n:npad] = 0.0
    A[np.arange(n, npad), np.arange(n, npad)] = 1.0  # the padding as the Gram kernel leaves it
    sw = rng.uniform(0.1, 2.0, n)
    got = gp.laplace_kernel_check("lap_scale_gram", 0, A=A, ld=ld, n=n, npad=npad, sw=sw, wcols=wcols).reshape(npad, ld)
    want = A.copy()
    ti = np.arange(npad) // 64
    low = (ti[:, None] >= ti[None, :])[:, :npad] & (np.arange(npad)[:, None] < n) & (np.arange(npad)[None, :] < n)
    sc = (sw[:, None] * A[:n, :n]) * sw[None, :]
    sc[np.arange(n), np.arange(n)] = 1.0 + sc[np.arange(n), np.arange(n)]
    want[:n, :n] = np.where(low[:n, :n], sc, A[:n, :n])
    assert same_bits(got, want)


@pytest.mark.parametrize("n", NS)
def test_step_kernels(n):
    npad = npad_of(n)
    rng = np.random.default_rng(n)
    z = np.full(npad, np.nan)
    for exact in (True, False):
        gen = (lambda k: dyadic(rng, k)) if exact else (lambda k: rng.normal(size=k))
        b, sw, beta, a, a1, f, f1 = (gen(n) for _ in range(7))
        rhs, ap = gp.laplace_kernel_check("lap_step", 0, b=b, sw=sw, beta=beta, n=n, npad=npad, rhs=z, a1=z)
        assert same_bits(rhs[:n], sw * beta) and not rhs[n:].any() and not ap[n:].any()
        for t in (1.0, 0.5, 0.25) if exact else (1.0, 0.3):
            at, ft = gp.laplace_kernel_check("lap_interp", 0, a=a, a1=a1, f=f, f1=f1, t=t, n=n, npad=npad, at=z, ft=z)
            assert not at[n:].any() and not ft[n:].any()
            if exact:
                assert same_bits(at[:n], a + t * (a1 - a)) and same_bits(ft[:n], f + t * (f1 - f))
            else:
                for got, u, v in ((at, a, a1), (ft, f, f1)):
                    assert (np.abs(got[:n] - (u + t * (v - u))) <= 4 * EPS * (np.abs(u) + np.abs(t * (v - u)))).all()
        if exact:
            assert same_bits(ap[:n], b - sw * beta)
        else:
            assert (np.abs(ap[:n] - (b - sw * beta)) <= 4 * EPS * (np.abs(b) + np.abs(sw * beta))).all()
    # t = 1 lands on the new iterate exactly where a1 - a is exact
    a, a1 = dyadic(rng, n), dyadic(rng, n)
    at, _ = gp.laplace_kernel_check("lap_interp", 0, a=a, a1=a1, f=a, f1=a1, t=1.0, n=n, npad=npad, at=z, ft=z)
    assert same_bits(at[:n], a1)


def lower_problem(n, rng, exact):
    """A symmetric matrix given by its lower triangle alone: NaN above the diagonal and on the padding, which no kernel
    may read"""
    npad, ld = npad_of(n), npad_of(n) + 8
    M = rng.integers(-4, 5, (n, n)).astype(float) if exact else rng.normal(size=(n, n))
    M = np.tril(M) + np.tril(M, -1).T
    A = np.full((npad, ld), np.nan)
    A[:n, :n] = np.where(np.tri(n, dtype=bool), M, np.nan)
    return npad, ld, M, A


@pytest.mark.parametrize("n", NS)
def test_weight_vector_and_symv(n):
    rng = np.random.default_rng(7 * n)
    for exact in (True, False):
        npad, ld, M, A = lower_problem(n, rng, exact)
        gen = (lambda k: rng.integers(-3, 4, k).astype(float)) if exact else (lambda k: rng.normal(size=k))
        rho, v, sv, sw = gen(n), gen(n), gen(n), gen(n)
        s = gp.laplace_kernel_check("lap_weight_vectors", 0, Binv=A, ld=ld, rho=rho, n=n, npad=npad, sv=np.full(npad, np.nan))
        assert same_bits(s[:n], 0.5 * (1.0 - np.diag(M)) * rho) and not s[n:].any()
        vp = np.concatenate([v, np.zeros(npad - n)])
        upart, u = gp.laplace_kernel_check("lap_symv_u", 0, Binv=A, ld=ld, n=n, npad=npad, v=vp, sv=sv, sw=sw,
                                           upart=np.full(npad // 64 * npad, np.nan), u=np.full(npad, np.nan))
        assert np.all(np.isfinite(upart)) and not u[n:].any()  # every (slot, row) is written, nothing above the diagonal read
        want = sv - sw * (M @ v)
        if exact:
            assert same_bits(u[:n], want)
        else:
            bound = (n + 8) * EPS * (np.abs(sv) + np.abs(sw) * (np.abs(M) @ np.abs(v)))
            print("symv n = %d: max err / bound = %.3f" % (n, (np.abs(u[:n] - want) / bound).max()))
            assert (np.abs(u[:n] - want) <= bound).all()


@pytest.mark.parametrize("n", NS)
def test_weight_kernel(n):
    rng = np.random.default_rng(11 * n)
    for exact in (True, False):
        npad, ld, M, A = lower_problem(n, rng, exact)
        A[np.isnan(A)] = 7.0  # in place: what is not the kernel's keeps its bits (NaN would not compare)
        gen = (lambda k: rng.integers(-3, 4, k).astype(float)) if exact else (lambda k: rng.normal(size=k))
        sw, u, a = gen(n), gen(n), gen(n)
        G = gp.laplace_kernel_check("lap_weight", 0, G=A, ld=ld, n=n, npad=npad, sw=sw, u=u, a=a).reshape(npad, ld)
        i, j = np.arange(npad)[:, None], np.arange(ld)[None, :]
        tiles = (i // 64 >= j // 64) & (j < npad)       # the lower 64-tiles: the kernel's
        inside = (i < n) & (j <= i)                      # ... and the elements the reduction reads
        assert same_bits(G[~tiles], A[~tiles])
        assert not G[tiles & ~inside].any()
        t1, t2, t3 = (sw[:, None] * M) * sw[None, :], np.outer(u, a), np.outer(a, u)
        want = t1 - t2 - t3
        low = np.tri(n, dtype=bool)
        if exact:
            assert same_bits(G[:n, :n][low], want[low])
        else:
            bound = 4 * EPS * (np.abs(t1) + np.abs(t2) + np.abs(t3))
            assert (np.abs(G[:n, :n] - want)[low] <= bound[low]).all()


@pytest.mark.parametrize("rows", [1, 64, 65, 300])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_colscale(n, rows):
    npad, ld = npad_of(n), npad_of(n) + 8
    rng = np.random.default_rng(n + rows)
    K = rng.normal(size=(rows, ld))
    sw = np.concatenate([rng.uniform(0.1, 2.0, n), np.zeros(npad - n)])
    got = gp.laplace_kernel_check("lap_colscale", 0, KsT=K, ld=ld, rows=rows, npad=npad, sw=sw).reshape(rows, ld)
    want = K.copy()
    want[:, :npad] = K[:, :npad] * sw[None, :]
    assert same_bits(got, want)


@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_mean_kernel(m):
    rng = np.random.default_rng(m)
    mu = np.concatenate([[0.0, 700.0, -700.0, 40.0, -40.0], rng.uniform(-6, 6, m)])[:m]
    sigma = np.concatenate([[0.0, 1.0, 1.0, 3.0, 0.0], rng.uniform(0, 3, m)])[:m]
    got = gp.laplace_kernel_check("lap_mean", 0, lik=LP.BERNOULLI, mu=mu, sigma=sigma, m=m, mean=np.full(m, np.nan))
    want = LP.gh_mean(LP.BERNOULLI, mu, sigma)
    # 32 positive terms; exp carries the rounding of its argument, |mu| + sqrt(2) sigma |x| <= |mu| + 10.1 sigma, twice
    # (the argument's own rounding and the fused product's)
    rtol = 1e-14 + 2 * EPS * (np.abs(mu) + 10.1 * sigma)
    print("mean m = %d bernoulli: max err / bound %.3f" % (m, (np.abs(got - want) / (rtol * want)).max()))
    assert np.all((got >= 0) & (got <= 1))
    assert (np.abs(got - want) <= rtol * want).all()
    mu = np.clip(mu, -300.0, 300.0)
    got = gp.laplace_kernel_check("lap_mean", 0, lik=LP.POISSON, mu=mu, sigma=sigma, m=m, mean=np.full(m, np.nan))
    arg = mu + 0.5 * sigma * sigma
    assert np.all(np.isfinite(got))
    assert (np.abs(got - np.exp(arg)) <= (1e-14 + 2 * EPS * np.abs(arg)) * np.exp(arg)).all()
    assert math.isclose(LP.GH_W.sum(), math.sqrt(math.pi), rel_tol=1e-15)
