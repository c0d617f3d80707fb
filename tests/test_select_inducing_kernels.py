"""The kernels of the greedy selection of inducing points (select.hip) in isolation, through gogp_test_select_step and
gogp_test_select_run.

One step, N in {1, 255, 257, 1000} x j in {0, 1, 37, 300} x max_blocks in {0, 1, 3} (the last two: workgroups that stride
over several row blocks, fewer partials than row blocks).  The columns of Lt and the pivot row hold small integers, so the
dot product is exact in any order; d_p = 4, so the division is exact; the padding rows of every column, the new column and
d / the factor's row of the rows selected earlier hold NaN on the way in: whatever leaks shows.

test_step_against_numpy: rows of a family's inputs, so that the only inexact term is k(x_i, x_p).
  new column: |l - l_ref| <= (D + 8) * 2.2e-16 * (|k| + |dot|) / sqrt(d_p) per element (the D accumulations of the distance
  plus the elementary functions' few ulp); d: twice that times |l|.  The rows' own d on the way in is l_ref^2 (1 + u),
  u in [0, 1): the result u l^2 is then small enough for the subtraction's own rounding (half an ulp of the result) to lie
  inside that bound -- |d_new| / 2 <= l^2 / 2 <= (D + 8) (|k| + |dot|) |l| since |l| <= (|k| + |dot|) / 2 -- where a d of
  order one beside a small l would leave nothing for it.  The step takes (p, d_p) from the partials it is handed, so these
  d need not stay below d_p.  Rows selected earlier and the pivot's own: exact 0 in d, exact 0 / 2 in the column.
  The new partials are compared EXACTLY with the per-workgroup maxima (lowest row first) of the d the device returned.
test_step_exact_with_ties: every row of X is the same point and the output scales sum to 2, so k = 2 exactly, l = (2 - dot) / 2
  and d - l^2 are exact: the column and d are compared with assert_array_equal.  d on the way in holds the value 4 at
  several rows of different workgroups (the pivot must be the lowest), and the new d has its maximum at rows of different
  workgroups and of different strides of one workgroup: the partials, and the pivot a following step takes from them,
  must name the lowest row.
test_run_*: the whole loop with the grid capped -- an integer initial diagonal with ties (piv[0] exact), and the same bits
  whatever the grid.

Reference counterpart: none."""
import numpy as np
import pytest

import grad_reduce_ref as GR
import select_inducing_ref as SI
from gogp_amd import _lib, kernel
from oracle.oracle import gram_np

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
NS, JS, MBS = [1, 255, 257, 1000], [0, 1, 37, 300], [0, 1, 3]
FAMS = SI.FOUR + ["ard_rbf64"]
NAN = np.nan


@pytest.fixture(scope="module")
def gpm():
    _lib.build()
    from gogp_amd import gp
    gp._lib.hooks()
    return gp


def _partials(gp, d, N, max_blocks):
    """(values, rows) of the workgroups' maxima of d, lowest row first; NaN counts as the largest."""
    nb = gp.select_blocks(N, max_blocks)
    owner = (np.arange(N) // 256) % nb
    v, ix = np.zeros(nb), np.zeros(nb, dtype=np.int64)
    for b in range(nb):
        rows = np.nonzero(owner == b)[0]
        k = rows[np.argmax(d[rows])]  # the first maximiser; the first NaN where there is one
        v[b], ix[b] = d[k], k
    return v, ix


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, float).view(np.int64), np.asarray(b, float).view(np.int64))


def _layout(N, j, rng, nsel):
    """ldn, Lt (j + 1 columns, NaN outside the live part), the selected rows and the pivot."""
    ldn = (N + 255) // 256 * 256 + (256 if j % 2 else 0)
    Lt = np.full((j + 1, ldn), NAN)
    Lt[:j, :N] = rng.integers(-3, 4, (j, N)).astype(float)
    rows = rng.permutation(N)
    sel = np.zeros(N, dtype=np.uint8)
    sel[rows[:nsel]] = 1
    Lt[:j, rows[:nsel]] = NAN  # the factor's rows of selected rows are not read
    return ldn, Lt, sel, rows[nsel:]


@pytest.mark.parametrize("max_blocks", MBS)
@pytest.mark.parametrize("j", JS)
@pytest.mark.parametrize("N", NS)
def test_step_against_numpy(gpm, N, j, max_blocks):
    name = FAMS[(NS.index(N) + JS.index(j)) % len(FAMS)]
    D, simil, ts = SI.FAMILIES[name]
    desc = kernel.build_desc(D, simil, SI.NOISE)
    ths = np.asarray(ts, float)
    kp = GR.kp_from_desc(desc, ths, SI.TN).hook(gpm)
    rng = np.random.default_rng(100 * N + j)
    X = SI.inputs(N, 1, D)[0]
    ldn, Lt, sel, free = _layout(N, j, rng, min(j, N - 1))
    p = int(free[0])
    k = gram_np(desc, ths, X, X[p:p + 1])[:, 0]
    with np.errstate(invalid="ignore"):
        dot = Lt[:j, :N].T @ Lt[:j, p] if j else np.zeros(N)
    l_ref = (k - dot) / 2.0
    d = l_ref * l_ref * (1.0 + rng.uniform(0.0, 1.0, N))
    d[sel == 1] = NAN
    d[p] = 4.0
    # the partials handed in: (4, p) from p's workgroup, a smaller value from the others
    nb = gpm.select_blocks(N, max_blocks)
    pv, pi = np.full(nb, 3.0), np.zeros(nb, dtype=np.int64)
    own = (p // 256) % nb
    for b in range(nb):
        pi[b] = min(b * 256, N - 1)
    pv[own], pi[own] = 4.0, p
    Lt2, d2, sel2, ov, oi, gp_, gdp = gpm.select_step_check(kp, X.reshape(-1), N, Lt.reshape(-1), ldn, j, 1e-8, d, sel, pv, pi,
                                                            max_blocks, device=0)
    Lt2 = Lt2.reshape(j + 1, ldn)
    assert gp_ == p and gdp == 4.0
    assert _same_bits(Lt2[:j], Lt[:j]) and np.all(np.isnan(Lt2[j, N:]))
    want_sel = sel.copy()
    want_sel[p] = 1
    np.testing.assert_array_equal(sel2, want_sel)
    col, live = Lt2[j, :N], (sel == 0)
    live[p] = False
    assert col[p] == 2.0 and d2[p] == 0.0
    assert np.all(col[sel == 1] == 0.0) and np.all(d2[sel == 1] == 0.0)
    tol = (D + 8) * EPS * (np.abs(k) + np.abs(dot)) / 2.0
    err = np.abs(col - l_ref)
    want_d = d - l_ref * l_ref
    errd = np.abs(d2 - want_d)
    print("%s N %d j %d max_blocks %d: column %.3g of its bound, d %.3g of its bound"
          % (name, N, j, max_blocks, (err[live] / tol[live]).max() if live.any() else 0.0,
             (errd[live] / (2 * tol[live] * np.abs(l_ref[live]) + 1e-300)).max() if live.any() else 0.0))
    assert np.all(err[live] <= tol[live])
    assert np.all(errd[live] <= 2 * tol[live] * np.abs(l_ref[live]))
    wv, wi = _partials(gpm, d2, N, max_blocks)
    np.testing.assert_array_equal(oi, wi)
    np.testing.assert_array_equal(ov, wv)


def _exact_kp(gpm, D, which):
    if which == 0:
        return gpm.kparams(D, [dict(kind=GR.K_MATERN52_TEXTBOOK, c=2.0, inv_len=0.7)])
    return gpm.kparams(D, [dict(kind=GR.K_MATERN32, c=1.0, inv_len=1.3), dict(kind=GR.K_PERIODIC, c=1.0, w=0.9, inv_len=0.6)])


@pytest.mark.parametrize("max_blocks", MBS)
@pytest.mark.parametrize("j", JS)
@pytest.mark.parametrize("N", NS)
def test_step_exact_with_ties(gpm, N, j, max_blocks):
    D = 2
    kp = _exact_kp(gpm, D, (N + j) % 2)
    rng = np.random.default_rng(7 * N + j)
    X = np.tile(np.array([0.3, -1.1]), N)  # one point N times: k = 2 exactly
    ties = sorted({N // 20, N // 10, (3 * N) // 10, (9 * N) // 10})  # N = 1000: rows 50, 100, 300, 900
    ldn, Lt, sel, free = _layout(N, j, rng, min(j, max(N - len(ties) - 1, 0)))
    for r in ties:  # the tied rows are live, with zero columns: dot = 0
        if sel[r]:
            sel[r] = 0
        Lt[:j, r] = 0.0
    live = sel == 0
    d = np.where(live, rng.integers(0, 3, N).astype(float), NAN)
    d[ties] = 4.0
    p = ties[0]
    pv, pi = _partials(gpm, np.where(live, d, -1.0), N, max_blocks)
    Lt2, d2, sel2, ov, oi, gp_, gdp = gpm.select_step_check(kp, X, N, Lt.reshape(-1), ldn, j, 0.0, d, sel, pv, pi,
                                                            max_blocks, device=0)
    Lt2 = Lt2.reshape(j + 1, ldn)
    assert gp_ == p and gdp == 4.0  # the lowest of the tied rows
    with np.errstate(invalid="ignore"):
        dot = Lt[:j, :N].T @ Lt[:j, p] if j else np.zeros(N)
    want_l = np.where(live, (2.0 - dot) / 2.0, 0.0)
    want_l[p] = 2.0
    want_d = np.where(live, d - want_l * want_l, 0.0)
    want_d[p] = 0.0
    np.testing.assert_array_equal(Lt2[j, :N], want_l)
    np.testing.assert_array_equal(d2, want_d)
    assert _same_bits(Lt2[:j], Lt[:j]) and np.all(np.isnan(Lt2[j, N:]))
    wv, wi = _partials(gpm, want_d, N, max_blocks)
    np.testing.assert_array_equal(oi, wi)
    np.testing.assert_array_equal(ov, wv)
    if N == 1:
        return
    # the other tied rows kept dot = 0: l = 1, d = 3, the maximum of the new d -- in different workgroups and (row 900
    # beside row 100 with three workgroups) in different strides of one
    top = np.nonzero(want_d == want_d.max())[0]
    assert want_d.max() == 3.0 and set(ties[1:]) <= set(top.tolist())
    if N == 1000:
        nb = gpm.select_blocks(N, max_blocks)
        owners = [(r // 256) % nb for r in ties[1:]]  # rows 100, 300, 900
        if nb == 3:
            assert owners[0] == owners[2] and owners[0] != owners[1]  # 900: workgroup 0's second stride
        elif nb == 4:
            assert len(set(owners)) == 3
    # a following step takes the lowest of them from those partials
    nxt = np.full((j + 2, ldn), NAN)
    nxt[:j + 1] = Lt2
    _, _, _, _, _, p1, dp1 = gpm.select_step_check(kp, X, N, nxt.reshape(-1), ldn, j + 1, 0.0, d2, sel2, ov, oi, max_blocks,
                                                   device=0)
    assert p1 == ties[1] and dp1 == 3.0


def test_step_stops_without_writing(gpm):
    """The best residual is not above tol, or is NaN: nothing is written and no pivot is recorded."""
    N, j, D = 300, 2, 2
    kp = _exact_kp(gpm, D, 0)
    X = np.tile(np.array([0.3, -1.1]), N)
    Lt = np.full((j + 1, 512), NAN)
    Lt[:j, :N] = 1.0
    sel = np.zeros(N, dtype=np.uint8)
    for d0, tol in ((np.full(N, 0.5), 0.5), (np.zeros(N), 0.0), (np.where(np.arange(N) == 270, NAN, 1.0), 1e-8)):
        pv, pi = _partials(gpm, d0, N, 0)
        Lt2, d2, sel2, ov, oi, p, dp = gpm.select_step_check(kp, X, N, Lt.reshape(-1), 512, j, tol, d0, sel, pv, pi, 0, device=0)
        assert p == -1
        assert _same_bits(Lt2, Lt.reshape(-1)) and _same_bits(d2, d0) and not sel2.any()
        assert np.all(np.isnan(ov)) and np.all(oi == -1)  # the wrapper's fill: the hook wrote none


@pytest.mark.parametrize("max_blocks", MBS)
@pytest.mark.parametrize("N", [257, 1000])
def test_run_integer_diagonal_with_ties(gpm, N, max_blocks):
    D, simil, ts = SI.FAMILIES["matern32_2d"]
    desc = kernel.build_desc(D, simil, SI.NOISE)
    kp = GR.kp_from_desc(desc, np.asarray(ts, float), SI.TN).hook(gpm)
    X = SI.inputs(N, 1, D)[0]
    rng = np.random.default_rng(N)
    d0 = rng.integers(1, 9, N).astype(float)
    tied = sorted({N // 5, N // 5 + 3, N - 20, N - 1})  # N = 1000: 200, 203 (one block), 980, 999 (another stride / workgroup)
    d0[tied] = 9.0
    idx, pv, U, L, d, trace = gpm.select_run_check(kp, X.reshape(-1), N, 5, 1e-8, max_blocks, d0, device=0)
    assert len(idx) == 5 and idx[0] == tied[0] and pv[0] == 9.0
    assert len(set(idx.tolist())) == 5
    np.testing.assert_array_equal(U, X[idx])
    assert np.all(d[idx] == 0.0)
    np.testing.assert_array_equal(np.diag(L[idx]), np.sqrt(pv))
    assert np.all(np.triu(L[idx], 1) == 0.0)


def test_run_does_not_depend_on_the_grid(gpm):
    """The rows' arithmetic does not depend on which workgroup takes them and the pivot rule is exact: the same bits for
    every cap of the grid.  Against the replay of the device's pivots in fp64 the factor agrees to rounding."""
    N, M = 1000, 40
    D, simil, ts = SI.FAMILIES["hyperpriors"]
    desc = kernel.build_desc(D, simil, SI.NOISE)
    ths = np.asarray(ts, float)
    kp = GR.kp_from_desc(desc, ths, SI.TN).hook(gpm)
    X = SI.inputs(N, 1, D)[0]
    base = gpm.select_run_check(kp, X.reshape(-1), N, M, 1e-8, 0, None, device=0)
    for mb in (1, 3):
        other = gpm.select_run_check(kp, X.reshape(-1), N, M, 1e-8, mb, None, device=0)
        for a, b in zip(base[:5], other[:5]):
            assert _same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)
        assert base[5] == other[5]
    idx, pv, U, L, d, trace = base
    assert len(idx) == M and idx[0] == 0
    K = gram_np(desc, ths, X, X)
    R, Lr = SI.replay(K, idx, np.float64)
    kmax = np.diag(K).max()
    # (the recurrence's own rounding is 1e-15 absolute; the last pivots are ~1e-4, and an error of d passes into l
    # through 1 / sqrt(d_p): 1e-10 of k(x, x) is far above both and far below any wrong row or column)
    assert np.abs(L - Lr).max() <= 1e-10 * kmax
    assert np.abs(d - R[-1]).max() <= 1e-10 * kmax
    assert abs(trace - d.sum()) <= N * EPS * kmax
