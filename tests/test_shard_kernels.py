"""The kernels of the sharded path and the rest of solve.hip, in isolation (run with -m gpu on the MI355X box): the
block-cyclic kernels of dist2d.hip and of the "helpers of the sharded evaluation" of solve.hip (chunk_alpha, chunk_rowsq +
sum, chunk_tdot + finish, gather_rows, gather_x, scatter_stage, scatter_tile, gather_rows_of_l, residual_block, copy_block),
the layout kernels and copies (transpose_sq, transpose_rect, pack_blocks, convert_block, zero_upper, ydiag, zero_block,
extract_lower, pack_lower, the one-line vector kernels) and the reductions (lml_scalars, alpha_from_y batched, trace_rows +
sum, dot, sumsq_info, logdet_block, sigma).

Everything goes through the PRODUCT launchers via the hooks of include/gogp_testhooks.h (gp.shard_kernel_check), which copy
whole host arrays to the device and back.  The three kinds of check of tests/test_substitution_kernels.py, with the
references, the layout model and the accuracy model of tests/shard_kernels_ref.py:
- exact: integer / dyadic operands -- BIT FOR BIT (copies, conversions and single IEEE operations on any operands too);
- full mantissa: random operands against the long-double evaluation of the same operations, |got - want| <= e (judge()
  asserts max(e) <= 1e-10 max |want|, so the bound cannot hide a failure);
- sentinels: NaNs with a payload in everything a launch must not read and everything it must not write; they come back bit
  for bit, and judge() fails on any non-finite result.
Every launch runs twice and must give the same bits; the reductions print their worst |err| / e on a RATIO line.
"""
import numpy as np
import pytest

import shard_kernels_ref as R
from cases import NAN32, NAN64
from gogp_amd import _lib
from test_substitution_kernels import bits, dtype_of, judge, nan_of, same_bits
from test_update_kernels import sentinels, untouched

pytestmark = pytest.mark.gpu
F64, F32, LD = np.float64, np.float32, np.longdouble
PRECS = [64, 32]


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def launch(gpm, which, **args):
    """The hook twice on the same arguments: the same bits both times."""
    a, b = gpm.shard_kernel_check(which, **args), gpm.shard_kernel_check(which, **args)
    several = isinstance(a, tuple)
    for x, y in zip(a if several else (a,), b if several else (b,)):
        assert same_bits(x, y), "%s: two identical launches differ in bits" % which
    return a


def filled(n, dt):
    return np.full(n, nan_of(dt), dt)


def kept(a, what):
    """Every element still holds its type's sentinel, bit for bit."""
    a = np.ascontiguousarray(a).reshape(-1)
    bad = np.flatnonzero(bits(a) != bits(filled(1, a.dtype))[0])
    assert bad.size == 0, "%s: %d of %d sentinels overwritten, first at %d" % (what, bad.size, a.size, bad[0])


def tail(a, dt=F64, n=5):
    """The flat array followed by sentinels: what lies behind an array a launch must neither read nor write."""
    return np.concatenate([np.ascontiguousarray(a, dt).reshape(-1), filled(n, dt)])


def strided(M, ld, dt=F64):
    """The matrix in rows of ld elements, sentinels in the padding columns, flat."""
    out = np.full((M.shape[0], ld), nan_of(dt), dt)
    out[:, :M.shape[1]] = M
    return out.reshape(-1)


def grid_map(nb_shift, Pr, Pc, pr, pc):
    return dict(nb_shift=nb_shift, Pr=Pr, Pc=Pc, pr=pr, pc=pc)


def all_ranks(Pr, Pc):
    return [(r, c) for r in range(Pr) for c in range(Pc)]


def layout_id(c):
    return "nb%d-%dx%d-x%d" % (1 << c[0], c[1], c[2], c[3])


# ---------------------------------------------------------------------------------------------------------------------
# the block-cyclic kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=layout_id)
def test_chunk_alpha(gpm, case, prec):
    nb_shift, Pr, Pc, mult = case
    dt, worst = dtype_of(prec), 0.0
    for exact in (True, False):
        p = R.layout_problem(nb_shift, Pr, Pc, mult, exact)
        nb, NB, npad = p["nb"], p["NB"], p["npad"]
        G, z = R.rounded(p["G"], prec), p["z"]
        total = np.zeros(npad)
        for pr, pc in (all_ranks(Pr, Pc) if exact else R.GRIDS[(Pr, Pc)]):
            Ych = R.chunks_of(G, nb, Pr, Pc, pr, pc, dt, R.upper)  # the chunks left of the diagonal hold sentinels
            out = launch(gpm, "chunk_alpha", precision=prec, Ych=Ych.reshape(-1), mloc=Ych.shape[1], nloc=Ych.shape[0],
                         z=z, out=sentinels(npad + 5), **grid_map(nb_shift, Pr, Pc, pr, pc))
            rows, want, e = R.chunk_alpha_ref(G, z, nb, Pr, Pc, pr, pc)
            assert np.array_equal(rows, R.global_rows(NB, nb, Pr, pr))
            worst = max(worst, judge(out[rows], want, None if exact else e, "chunk_alpha rank (%d, %d)" % (pr, pc)))
            mask = np.ones(npad + 5, bool)
            mask[rows] = False
            untouched(out[mask], "out off this rank's rows")
            total[rows] += out[rows]
        if exact:  # the partial sums of a grid add up to the block-upper-triangular product
            Gu = G * (np.arange(npad)[:, None] // nb <= np.arange(npad)[None, :] // nb)
            assert same_bits(total, Gu @ z), "the ranks' partial sums do not add up to Y z"
    print("RATIO chunk_alpha %s prec%d %.4f" % (layout_id(case), prec, worst))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.SUMSQ_CASES, ids=layout_id)
def test_chunk_sumsq(gpm, case, prec):
    nb_shift, Pr, Pc, mult = case
    dt, worst = dtype_of(prec), 0.0
    for exact in (True, False):
        p = R.layout_problem(nb_shift, Pr, Pc, mult, exact)
        nb, NB, npad = p["nb"], p["NB"], p["npad"]
        G = R.rounded(p["G"], prec)
        ns = R.sumsq_ns(nb, npad) if nb_shift == 6 else [npad - nb // 2 - 1]
        for n in ns:
            Gn = G.copy()
            Gn[n:] = np.nan  # rows >= n contribute exactly 0 even where the chunks hold NaN: they are never read
            total = 0.0
            for pr, pc in (all_ranks(Pr, Pc) if exact else R.GRIDS[(Pr, Pc)]):
                Ych = R.chunks_of(Gn, nb, Pr, Pc, pr, pc, dt, R.upper)
                lrows = Ych.shape[1] * nb
                part, out = launch(gpm, "chunk_sumsq", precision=prec, Ych=Ych.reshape(-1), mloc=Ych.shape[1],
                                   nloc=Ych.shape[0], n=n, part=sentinels(lrows + 5), out=sentinels(6),
                                   **grid_map(nb_shift, Pr, Pc, pr, pc))
                (wp, wo), (ep, eo) = R.chunk_sumsq_ref(G, nb, Pr, Pc, pr, pc, n)
                what = "chunk_sumsq n%d rank (%d, %d)" % (n, pr, pc)
                dead = R.global_rows(NB, nb, Pr, pr) >= n
                assert same_bits(part[:lrows][dead], np.zeros(int(dead.sum()))), what + ": a row >= n is not exactly +0.0"
                if wo[0] == 0:
                    assert same_bits(out[:1], np.zeros(1)), what
                    assert same_bits(part[:lrows], np.zeros(lrows)), what
                else:
                    worst = max(worst, judge(part[:lrows], wp, None if exact else ep, what + " part"))
                    worst = max(worst, judge(out[:1], wo, None if exact else eo, what + " out"))
                untouched(part[lrows:], "part behind the local rows")
                untouched(out[1:], "out behind the sum")
                total += out[0]
            if exact:
                Gu = G[:n] * (np.arange(n)[:, None] // nb <= np.arange(npad)[None, :] // nb)
                assert total == (Gu ** 2).sum(), "the ranks' sums do not add up to |Y|_F^2 over the rows < n"
    print("RATIO chunk_sumsq %s prec%d %.4f" % (layout_id(case), prec, worst))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nb", R.TDOT_NB)
@pytest.mark.parametrize("rows", R.TDOT_ROWS)
def test_chunk_tdot(gpm, rows, nb, prec):
    dt, worst = dtype_of(prec), 0.0
    scratch = gpm.chunk_tdot_scratch(rows, nb)
    nslab = -(-rows // R.TDOT_SLAB)
    assert scratch >= nslab * nb
    for exact in (True, False):
        p = R.tdot_problem(rows, nb, exact)
        C = R.rounded(p["C"], prec)
        part, out = launch(gpm, "chunk_tdot", precision=prec, chunk=tail(C, dt, 3 * nb), rows=rows, nb=nb,
                           v=tail(p["v"]), part=sentinels(scratch + 5), out=sentinels(nb + 5))
        (wp, wo), (ep, eo) = R.tdot_ref(C, p["v"])
        worst = max(worst, judge(part[:nslab * nb].reshape(nslab, nb), wp, None if exact else ep, "part"))
        worst = max(worst, judge(out[:nb], wo, None if exact else eo, "out"))
        untouched(part[nslab * nb:], "the slabs beyond the last one")
        untouched(out[nb:], "out behind nb")
    print("RATIO chunk_tdot rows%d nb%d prec%d %.4f" % (rows, nb, prec, worst))


@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=layout_id)
def test_gather_rows_and_x(gpm, case):
    nb_shift, Pr, Pc, mult = case
    nb, NB = 1 << nb_shift, R.num_tiles(Pr, Pc, mult)
    npad = NB * nb
    rng = np.random.default_rng(21)
    y = rng.standard_normal(npad)
    for pr, pc in R.GRIDS[(Pr, Pc)]:
        g = R.global_rows(NB, nb, Pr, pr)
        yloc = launch(gpm, "gather_rows", y=y, rows=len(g), yloc=sentinels(len(g) + 5), **grid_map(nb_shift, Pr, Pc, pr, pc))
        assert same_bits(yloc[:len(g)], y[g])
        untouched(yloc[len(g):], "yloc behind the local rows")
        for D in (1, 3):
            for n in (npad - nb // 2 - 1, 1, npad):
                X, a = rng.standard_normal((n, D)), rng.standard_normal(n)
                Xloc, aloc = launch(gpm, "gather_x", X=tail(X), a=tail(a), D=D, n=n, rows=len(g),  # NaN from row n on
                                    Xloc=sentinels(len(g) * D + 5), aloc=sentinels(len(g) + 5),
                                    **grid_map(nb_shift, Pr, Pc, pr, pc))
                live = g < n
                wX, wa = np.zeros((len(g), D)), np.zeros(len(g))
                wX[live], wa[live] = X[g[live]], a[g[live]]
                assert same_bits(Xloc[:len(g) * D], wX.reshape(-1)) and same_bits(aloc[:len(g)], wa), (D, n, pr, pc)
                untouched(Xloc[len(g) * D:], "Xloc behind the local rows")
                untouched(aloc[len(g):], "aloc behind the local rows")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=layout_id)
def test_scatter_stage(gpm, case, prec):
    nb_shift, Pr, Pc, mult = case
    nb, NB, dt = 1 << nb_shift, R.num_tiles(Pr, Pc, mult), dtype_of(prec)
    mloc, nloc = NB // Pr, NB // Pc
    rng = np.random.default_rng(22)
    lds = nloc * nb + 8
    for bi in range(mloc):
        stage = rng.standard_normal((nb, nloc * nb))  # full mantissas: the float instance has to round
        Lch = launch(gpm, "scatter_stage", precision=prec, stage=tail(strided(stage, lds)), lds=lds,
                     Lch=filled(nloc * mloc * nb * nb + 5, dt), nloc=nloc, mloc=mloc, bi=bi, nb=nb)
        tiles = Lch[:nloc * mloc * nb * nb].reshape(nloc, mloc, nb, nb)
        for bj in range(nloc):  # every (bj, bi, r, c) of the layout [bj][bi][r][c]
            assert same_bits(np.ascontiguousarray(tiles[bj, bi]), stage[:, bj * nb:(bj + 1) * nb].astype(dt)), (bi, bj)
        kept(np.delete(tiles, bi, axis=1), "the tiles of other local rows")
        kept(Lch[nloc * mloc * nb * nb:], "Lch behind the chunks")


SCATTER_TILE = [  # nb, n, row0, col0, diag, r0
    (64, 165, 128, 128, 1, 64), (64, 165, 128, 64, 0, 64), (64, 165, 64, 64, 1, 64), (64, 165, 64, 0, 0, 0),
    (64, 165, 0, 0, 1, 0), (64, 165, 128, 0, 0, 128), (64, 64, 0, 0, 1, 0), (64, 1, 0, 0, 1, 0),
    (512, 700, 512, 512, 1, 512), (512, 700, 512, 0, 0, 0)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nb,n,row0,col0,diag,r0", SCATTER_TILE)
def test_scatter_tile(gpm, nb, n, row0, col0, diag, r0, prec):
    dt = dtype_of(prec)
    rng = np.random.default_rng(23)
    src = rng.standard_normal((nb, nb)).astype(dt)
    rend = min(row0 + nb, n)
    seen = src.copy()
    seen[rend - row0:] = nan_of(dt)  # rows and columns at or beyond n are not read
    seen[:, max(min(n - col0, nb), 0):] = nan_of(dt)
    if diag:
        seen[np.triu_indices(nb, 1)] = nan_of(dt)  # nor what lies above the diagonal of a diagonal tile
    band = (rend - r0) * n
    dst = launch(gpm, "scatter_tile", precision=prec, src=seen.reshape(-1), nb=nb, n=n, row0=row0, col0=col0, diag=diag,
                 r0=r0, dst=sentinels(band + 5))
    want = np.full((rend - r0, n), NAN64)
    for r in range(row0, rend):
        c1 = min(col0 + nb, n, r + 1 if diag else n)
        want[r - r0, col0:c1] = src[r - row0, :c1 - col0]
    assert same_bits(dst[:band], want.reshape(-1))  # (the sentinels of `want` are what must stay untouched)
    untouched(dst[band:], "dst behind the band")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=layout_id)
def test_gather_rows_of_l(gpm, case, prec):
    nb_shift, Pr, Pc, mult = case
    dt = dtype_of(prec)
    p = R.layout_problem(nb_shift, Pr, Pc, mult, False)
    nb, npad = p["nb"], p["npad"]
    n = npad - nb // 2 - 1
    L = R.rounded(p["G"], prec).copy()
    L[np.triu_indices(npad, 1)] = np.nan  # never read: above the diagonal, and the padding rows and columns
    L[n:], L[:, n:] = np.nan, np.nan
    # unsorted, repeated, 0, n - 1, the first and last row of a tile
    rows = np.array([r % n for r in (5, n - 1, 0, 5, nb - 1, nb, npad - nb, n - 1, npad - nb - 1)], np.int64)
    full, count = np.zeros((len(rows), n)), np.zeros((len(rows), n), int)
    dfull, dcount = np.zeros(n), np.zeros(n, int)
    for pr, pc in all_ranks(Pr, Pc):
        Lch = R.chunks_of(L, nb, Pr, Pc, pr, pc, dt, R.lower)
        a = dict(precision=prec, Lch=Lch.reshape(-1), mloc=Lch.shape[1], nloc=Lch.shape[0], n=n,
                 **grid_map(nb_shift, Pr, Pc, pr, pc))
        out = launch(gpm, "gather_rows_of_l", rows=rows, diag_only=0, out=sentinels(len(rows) * n + 5), **a)
        untouched(out[len(rows) * n:], "out behind the rows")
        o = out[:len(rows) * n].reshape(len(rows), n)
        wrote = bits(o) != bits(sentinels(1))[0]
        mine = np.array([[(r // nb) % Pr == pr and (c // nb) % Pc == pc and c <= r for c in range(n)] for r in rows])
        assert np.array_equal(wrote, mine), "rank (%d, %d) wrote other than what its tiles hold" % (pr, pc)
        full[wrote] += o[wrote]
        count += wrote
        dg = launch(gpm, "gather_rows_of_l", rows=None, diag_only=1, out=sentinels(n + 5), **a)
        untouched(dg[n:], "the diagonal behind n")
        wrote = bits(dg[:n]) != bits(sentinels(1))[0]
        dfull[wrote] += dg[:n][wrote]
        dcount += wrote
    tri = np.array([[c <= r for c in range(n)] for r in rows])
    assert np.array_equal(count, tri.astype(int)), "the ranks do not cover the requested rows exactly once"
    assert same_bits(full[tri], L[rows][:, :n][tri]) and not full[~tri].any()
    assert (dcount == 1).all() and same_bits(dfull, np.diag(L)[:n].copy())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nrecv", R.RESIDUAL_NRECV)
@pytest.mark.parametrize("rows", R.RESIDUAL_ROWS)
@pytest.mark.parametrize("nb", [64, 512])
def test_residual_block_and_copy_block(gpm, nb, rows, nrecv, prec):
    rows = nb + 3 if rows is None else rows
    dt, ld, worst = dtype_of(prec), 2 * nb + 8, 0.0
    for exact in (True, False):
        p = R.residual_problem(rows, nb, nrecv, exact)
        Ks, U, recv = R.rounded(p["Ks"], prec), p["U"], p["recv"]
        W = launch(gpm, "residual_block", precision=prec, W=filled(rows * nb + 5, dt), Ks=strided(Ks, ld, dt),
                   U=strided(U, ld), ld=ld, recv=tail(recv) if nrecv else None, nrecv=nrecv, nb=nb, rows=rows)
        kept(W[rows * nb:], "W behind the block")
        got = W[:rows * nb].reshape(rows, nb)
        in_order = R.residual_eval(Ks, U, recv, F64)  # single IEEE operations in the kernel's order: the same bits
        if prec == 32:  # rounded once, from the fp64 difference
            assert same_bits(np.ascontiguousarray(got), in_order.astype(F32)), "not ONE rounding of the fp64 difference"
        elif exact:
            judge(got, R.residual_eval(Ks, U, recv, LD), None, "residual_block")
        else:
            want, e = R.residual_ref(Ks, U, recv)
            worst = max(worst, judge(got, want, e, "residual_block"))
        if prec == 64 and nrecv == 0:
            dst = launch(gpm, "copy_block", dst=sentinels(rows * nb + 5), src=strided(U, ld), ld=ld, nb=nb, rows=rows)
            assert same_bits(dst[:rows * nb], U.reshape(-1))
            untouched(dst[rows * nb:], "dst behind the block")
    print("RATIO residual_block nb%d rows%d nrecv%d prec%d %.4f" % (nb, rows, nrecv, prec, worst))


# ---------------------------------------------------------------------------------------------------------------------
# layout and copies
# ---------------------------------------------------------------------------------------------------------------------
def coded(rows, cols, dt):
    """Data that encodes (i, j), exact in float."""
    return (np.arange(rows)[:, None] * 4096.0 + np.arange(cols)[None, :] + 1.0).astype(dt)


def check_transposed(dst, src, ldd, dt):
    rows, cols = src.shape
    d = dst[:cols * ldd].reshape(cols, ldd)
    assert same_bits(np.ascontiguousarray(d[:, :rows]), np.ascontiguousarray(src.T))
    kept(d[:, rows:], "the padding columns of dst")
    kept(dst[cols * ldd:], "dst behind the last row")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", R.TRANSPOSE_SQ_N)
def test_transpose_sq(gpm, n, prec):
    dt, lds, ldd = dtype_of(prec), n + 8, n + 24
    src = coded(n, n, dt)
    dst = launch(gpm, "transpose_sq", precision=prec, src=tail(strided(src, lds, dt), dt), lds=lds,
                 dst=filled(n * ldd + 5, dt), ldd=ldd, n=n)
    check_transposed(dst, src, ldd, dt)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_RECT)
def test_transpose_rect(gpm, rows, cols, prec):
    dt, lds, ldd = dtype_of(prec), cols + 8, rows + 24
    src = coded(rows, cols, dt)
    dst = launch(gpm, "transpose_rect", precision=prec, src=tail(strided(src, lds, dt), dt), lds=lds,
                 dst=filled(cols * ldd + 5, dt), ldd=ldd, rows=rows, cols=cols)
    check_transposed(dst, src, ldd, dt)


@pytest.mark.parametrize("half", R.PACK_HALF_BLK)
def test_pack_blocks(gpm, half):
    blk, nblk, first, stride = 2 * half, 3, 1, 3
    nsrc = first + (nblk - 1) * stride + 1
    rng = np.random.default_rng(24)
    src = np.full((nsrc, blk), NAN64)  # the unselected blocks are never read: their bits would show in dst
    sel = [first + d * stride for d in range(nblk)]
    src[sel] = rng.integers(0, 2 ** 64, (nblk, blk), dtype=np.uint64).view(F64)  # any bits: floats travel as doubles
    odd = np.array([0x7FF0000000000001, 0xFFF8000000000123, 0x7FC0BEEF7FC0BEEF, 0x0000000000000001], np.uint64).view(F64)
    src[sel[1], :min(4, blk)] = odd[:min(4, blk)]  # payload NaNs, two float NaNs in one double, a denormal
    dst = launch(gpm, "pack_blocks", dst=sentinels(nblk * blk + 5), src=src.reshape(-1), nblk=nblk, blk=blk, first=first,
                 stride=stride)
    assert same_bits(dst[:nblk * blk], src[sel].reshape(-1))
    untouched(dst[nblk * blk:], "the destination's tail")


@pytest.mark.parametrize("p_src,p_dst", [(32, 64), (64, 32), (64, 64)])
@pytest.mark.parametrize("rows", R.CONVERT_ROWS)
@pytest.mark.parametrize("cols", R.CONVERT_COLS)
def test_convert_block(gpm, cols, rows, p_src, p_dst):
    ds, dd, lds, ldd = dtype_of(p_src), dtype_of(p_dst), cols + 3, cols + 7
    src = np.random.default_rng(25).standard_normal((rows, cols)).astype(ds)  # (doubles that need rounding)
    dst = launch(gpm, "convert_block", precision=p_src, precision2=p_dst, src=tail(strided(src, lds, ds), ds), lds=lds,
                 dst=filled(rows * ldd + 5, dd), ldd=ldd, rows=rows, cols=cols)
    d = dst[:rows * ldd].reshape(rows, ldd)
    assert same_bits(np.ascontiguousarray(d[:, :cols]), src.astype(dd))
    kept(d[:, cols:], "the padding columns of dst")
    kept(dst[rows * ldd:], "dst behind the last row")


def batched(one, k, stride, dt, extra=5):
    """k flat arrays `stride` elements apart in one arena of sentinels."""
    arena = filled((k - 1) * stride + len(one[0]) + extra, dt)
    for c, a in enumerate(one):
        arena[c * stride:c * stride + len(a)] = a
    return arena


@pytest.mark.parametrize("prec,k", [(64, 1), (64, 2), (32, 1)])
@pytest.mark.parametrize("npad", R.ZERO_UPPER_NPAD)
def test_zero_upper_blocks(gpm, npad, prec, k):
    dt, ld = dtype_of(prec), npad + 8
    rng = np.random.default_rng(26)
    mats = [rng.standard_normal((npad, ld)).astype(dt) for _ in range(k)]
    stride = npad * ld + 6
    R0 = batched([m.reshape(-1) for m in mats], k, stride, dt)
    out = launch(gpm, "zero_upper_blocks", precision=prec, R=R0, ld=ld, npad=npad, k=k, bstride=stride if k > 1 else 0)
    blk = np.arange(npad) // 256
    up = np.zeros((npad, ld), bool)
    up[:, :npad] = blk[None, :] > blk[:, None]  # strictly upper 256-blocks; the padding columns are not among them
    want = R0.copy()
    for c, m in enumerate(mats):
        w = m.copy()
        w[up] = 0.0
        want[c * stride:c * stride + npad * ld] = w.reshape(-1)
    assert same_bits(out, want)  # +0.0 there; diagonal blocks, lower part, padding and gaps bit for bit
    if npad == 256:
        assert same_bits(out, R0)


@pytest.mark.parametrize("prec,k", [(64, 1), (64, 2), (32, 1)])
def test_ydiag(gpm, prec, k):
    dt, ld = dtype_of(prec), 264
    D = [coded(256, 256, dt) + c * 0.5 for c in range(k)]  # asymmetric
    stride = 256 * ld + 10
    Y = launch(gpm, "ydiag", precision=prec, Dinv=batched([d.reshape(-1) for d in D], k, stride, dt, 0),
               Y=filled((k - 1) * stride + 256 * ld + 5, dt), ld=ld, k=k, bstride=stride if k > 1 else 0)
    want = filled(len(Y), dt)
    for c in range(k):
        w = np.full((256, ld), nan_of(dt), dt)
        w[:, :256] = D[c].T
        want[c * stride:c * stride + 256 * ld] = w.reshape(-1)
    assert same_bits(Y, want)


@pytest.mark.parametrize("prec,k", [(64, 1), (64, 2), (32, 1)])
@pytest.mark.parametrize("cols", R.ZERO_BLOCK_COLS)
def test_zero_block(gpm, cols, prec, k):
    dt, ld, rows = dtype_of(prec), 520, 3
    rng = np.random.default_rng(27)
    mats = [rng.standard_normal((rows, ld)).astype(dt) for _ in range(k)]
    stride = rows * ld + 6
    B0 = batched([m.reshape(-1) for m in mats], k, stride, dt)
    out = launch(gpm, "zero_block", precision=prec, B=B0, ld=ld, rows=rows, cols=cols, k=k, bstride=stride if k > 1 else 0)
    want = B0.copy()
    for c, m in enumerate(mats):
        w = m.copy()
        w[:, :cols] = 0.0
        want[c * stride:c * stride + rows * ld] = w.reshape(-1)
    assert same_bits(out, want)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", R.EXTRACT_N)
def test_extract_lower(gpm, n, prec):
    dt, ld = dtype_of(prec), n + 5
    L = np.random.default_rng(28).standard_normal((n, n)).astype(dt)
    Lf = L.copy()
    Lf[np.triu_indices(n, 1)] = nan_of(dt)  # the upper triangle is never read
    out = launch(gpm, "extract_lower", precision=prec, L=tail(strided(Lf, ld, dt), dt), ld=ld, n=n, out=sentinels(n * n + 5))
    assert same_bits(out[:n * n], np.tril(L).astype(F64).reshape(-1) + 0.0)  # exact +0.0 above the diagonal
    untouched(out[n * n:], "out behind the matrix")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,npad", R.PACK_LOWER)
def test_pack_lower(gpm, n, npad, prec):
    dt, ld = dtype_of(prec), npad + 8
    A = np.random.default_rng(29).standard_normal((n, n))
    Af = A.copy()
    Af[np.triu_indices(n, 1)] = NAN64  # never read
    L = launch(gpm, "pack_lower", precision=prec, src=tail(Af), n=n, npad=npad, L=filled(npad * ld + 5, dt), ld=ld)
    Lm = L[:npad * ld].reshape(npad, ld)
    want = np.eye(npad)
    want[:n, :n] = np.tril(A)
    assert same_bits(np.ascontiguousarray(Lm[:, :npad]), want.astype(dt))  # rounded once; the padding is the identity
    kept(Lm[:, npad:], "the columns >= npad of L")
    kept(L[npad * ld:], "L behind the last row")


def vector_op(gpm, op, a, b, count, f=0.0, prec=64):
    dt = dtype_of(prec)
    return launch(gpm, "vector_op", op=_lib.VECTOR_OPS[op], precision=prec, a=tail(a, dt),
                  b=None if b is None else tail(b, dt), count=count, f=f)


@pytest.mark.parametrize("count", R.VECTOR_COUNTS + [R.ADD_INPLACE_WRAP, R.FILL_WRAP])
def test_vector_ops(gpm, count):
    rng = np.random.default_rng(30)
    a, b, f = rng.standard_normal(count), rng.standard_normal(count), 1.0 / 3.0
    wrap = count > 1000  # past the capped grids: the two grid-stride kernels alone
    ops = {"fill": np.full(count, f), "add_inplace": a + b}
    if not wrap:
        ops.update(axpy=a + b, add_vec=a + b, scale=a * f, residual_from=b - a)
    for op, want in ops.items():  # single IEEE operations: the same bits as numpy's
        got = vector_op(gpm, op, a, None if op in ("fill", "scale") else b, count, f)  # (these two take no b)
        assert same_bits(got[:count], want), op
        untouched(got[count:], op + ": behind count")
    a32, b32 = a.astype(F32), b.astype(F32)
    got = vector_op(gpm, "add_inplace", a32, b32, count, prec=32)
    assert same_bits(got[:count], a32 + b32)
    kept(got[count:], "add_inplace<float>: behind count")


@pytest.mark.parametrize("v", [0, 1, -1, 2 ** 53 + 1, 123456789])
def test_info_to_double(gpm, v):
    got = vector_op(gpm, "info_to_double", np.zeros(1), np.array([v], np.int64).view(F64), 1)
    assert same_bits(got[:1], np.array([float(v)]))
    untouched(got[1:], "behind the word")


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------
def lml_arrays(p, n, ld, prec):
    dt = dtype_of(prec)
    L = np.full((n, ld), nan_of(dt), dt)  # NaN everywhere off the diagonal
    L[np.arange(n), np.arange(n)] = p["d"]
    return L.reshape(-1), R.rounded(p["d"], prec)


def check_scalars(got, p, d, with_alpha, exact, what):
    want, e = R.lml_ref(d, p["z"], p["y"], p["a"] if with_alpha else None)
    ratio = judge(got[:1], want[:1], e[:1], what + " log-determinant")  # held to the log model, exact operands too
    if exact:
        judge(got[1:3], want[1:3], None, what + " z'z, y'alpha")
    else:
        ratio = max(ratio, judge(got[1:2], want[1:2], e[1:2], what + " z'z"))
        if with_alpha:
            ratio = max(ratio, judge(got[2:3], want[2:3], e[2:3], what + " y'alpha"))
    if not with_alpha:
        assert same_bits(got[2:3], np.zeros(1)), what + ": slot 2 is not exactly 0 without alpha"
    assert same_bits(got[3:5], np.array([d.min(), d.max()])), what + ": min / max pivot"
    return ratio


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", R.LML_N)
def test_lml_scalars(gpm, n, prec):
    ld, worst = n + 3, 0.0
    for exact in (True, False):
        p = R.lml_problem(n, exact)
        L, d = lml_arrays(p, n, ld, prec)
        for with_alpha in (False, True):
            got = launch(gpm, "lml_scalars", precision=prec, L=L, ld=ld, z=tail(p["z"]), y=tail(p["y"]),
                         alpha=tail(p["a"]) if with_alpha else None, n=n, k=1, bstride=0, scalars=sentinels(8))
            untouched(got[5:], "scalars[5..]")
            worst = max(worst, check_scalars(got, p, d, with_alpha, exact, "lml_scalars n%d" % n))
    print("RATIO lml_scalars n%d prec%d %.4f" % (n, prec, worst))


@pytest.mark.parametrize("n", R.LML_BATCHED_N)
def test_lml_scalars_batched(gpm, n):
    k, ld, worst = R.BATCH_K, n + 3, 0.0
    stride = n * ld + 2
    for exact in (True, False):
        ps = [R.lml_problem(n, exact, seed=c + 1) for c in range(k)]  # every candidate its own data; y is shared
        y = ps[0]["y"]
        for with_alpha in (False, True):
            got = launch(gpm, "lml_scalars", precision=64, L=batched([lml_arrays(p, n, ld, 64)[0] for p in ps], k, stride, F64),
                         ld=ld, z=batched([p["z"] for p in ps], k, stride, F64), y=tail(y),
                         alpha=batched([p["a"] for p in ps], k, stride, F64) if with_alpha else None, n=n, k=k,
                         bstride=stride, scalars=sentinels((k - 1) * stride + 8))
            for c, p in enumerate(ps):
                q = dict(p, y=y)
                worst = max(worst, check_scalars(got[c * stride:c * stride + 5], q, p["d"], with_alpha, exact,
                                                 "candidate %d" % c))
                untouched(got[c * stride + 5:(c + 1) * stride if c + 1 < k else None], "behind candidate %d's scalars" % c)
    print("RATIO lml_scalars_batched n%d %.4f" % (n, worst))


@pytest.mark.parametrize("npad", [256, 512])
def test_alpha_from_y_batched(gpm, npad):
    k, ld, worst = R.BATCH_K, npad + 8, 0.0
    stride = npad * ld + 2
    mask = R.block_mask(npad, npad)
    for exact in (True, False):
        ps = [R.rowblock_problem(npad, npad, exact, seed=c + 1) for c in range(k)]
        Ys = [strided(np.where(mask, p["Y"], NAN64), ld) for p in ps]  # left of the row's block: never read
        got = launch(gpm, "alpha_from_y_batched", Y=batched(Ys, k, stride, F64), ld=ld,
                     z=batched([p["z"] for p in ps], k, stride, F64), npad=npad, k=k, bstride=stride,
                     alpha=sentinels((k - 1) * stride + npad + 5))
        for c, p in enumerate(ps):
            want, e = R.alpha_ref(p["Y"], p["z"])
            worst = max(worst, judge(got[c * stride:c * stride + npad], want, None if exact else e, "candidate %d" % c))
            untouched(got[c * stride + npad:(c + 1) * stride if c + 1 < k else None], "behind candidate %d's alpha" % c)
    print("RATIO alpha_from_y_batched npad%d %.4f" % (npad, worst))


@pytest.mark.parametrize("n", R.TRACE_N)
def test_trace_from_y(gpm, n):
    npad, worst = R.up256(n), 0.0
    ld = npad + 8
    mask = R.block_mask(n, npad)
    for exact in (True, False):
        p = R.rowblock_problem(n, npad, exact)
        Y = p["Y"].astype(F32)  # the columns n .. npad - 1 hold data: the launch reads them
        part, out = launch(gpm, "trace_from_y", Y=strided(np.where(mask, Y, NAN32), ld, F32), ld=ld, n=n, npad=npad,
                           alpha=tail(p["a"]), part=sentinels(n + 5), out=sentinels(6))
        (wp, wo), (ep, eo) = R.trace_ref(Y.astype(F64), p["a"])
        worst = max(worst, judge(part[:n], wp, None if exact else ep, "part"))
        worst = max(worst, judge(out[:1], wo, None if exact else eo, "out"))
        untouched(part[n:], "part behind n")
        untouched(out[1:], "out behind the trace")
    print("RATIO trace_from_y n%d %.4f" % (n, worst))


@pytest.mark.parametrize("n", R.REDUCE_N)
def test_dot_and_sumsq_info(gpm, n):
    worst = 0.0
    for exact in (True, False):
        p = R.vec_problem(n, exact)
        out = launch(gpm, "dot", a=tail(p["a"]), b=tail(p["b"]), n=n, out=sentinels(6))
        want, e = R.dot_ref(p["a"], p["b"])
        worst = max(worst, judge(out[:1], want, None if exact else e, "dot"))
        untouched(out[1:], "dot: out behind the sum")
        want, e = R.dot_ref(p["a"], p["a"])
        for info in (None, np.array([n + 7], np.int64)):
            out = launch(gpm, "sumsq_info", z=tail(p["a"]), n=n, info=info, out=sentinels(7))
            worst = max(worst, judge(out[:1], want, None if exact else e, "sumsq_info"))
            if info is None:
                untouched(out[1:], "sumsq_info without info: out[1..]")
            else:
                assert out[1] == float(n + 7)
                untouched(out[2:], "sumsq_info: out[2..]")
    print("RATIO dot_sumsq_info n%d %.4f" % (n, worst))


@pytest.mark.parametrize("nb", [64, 512])
@pytest.mark.parametrize("live", ["middle", "all", "none", "one"])
def test_logdet_block(gpm, nb, live):
    row0, ld, acc0 = 2 * nb, nb + 8, 3.25
    nlive = {"middle": nb // 2 + 3, "all": nb, "none": 0, "one": 1}[live]
    n = {"middle": row0 + nlive, "all": row0 + nb + 9, "none": row0, "one": row0 + 1}[live]
    d = np.random.default_rng(31).uniform(1.5, 4.0, nb)
    L = np.full((nb, ld), NAN64)
    L[np.arange(nlive), np.arange(nlive)] = d[:nlive]  # the diagonal from row n on is not read either
    acc = launch(gpm, "logdet_block", L=L.reshape(-1), ld=ld, row0=row0, n=n, nb=nb, acc=tail(np.array([acc0])))
    want, e = R.logdet_ref(d, nlive, acc0)
    ratio = judge(acc[:1], want, e, "logdet_block")
    if nlive == 0:
        assert same_bits(acc[:1], np.array([acc0]))
    untouched(acc[1:], "behind the accumulator")
    print("RATIO logdet_block nb%d %s %.4f" % (nb, live, ratio))


@pytest.mark.parametrize("m", R.SIGMA_M)
def test_sigma(gpm, m):
    worst = 0.0
    for exact in (True, False):
        p = R.sigma_problem(m, exact)
        for q in (None, p["q"]):
            prior = p["prior"] if q is not None else p["prior"] - p["q"]
            s = launch(gpm, "sigma", prior=tail(prior), q=None if q is None else tail(q), m=m, sigma=sentinels(m + 5))
            want, e = R.sigma_ref(prior, q)
            worst = max(worst, judge(s[:m], want, None if exact else e, "sigma"))
            untouched(s[m:], "sigma behind m")
    # prior < q: the root of a negative number, NaN -- unclamped, as the reference library leaves it
    prior, q = np.array([1.0, 4.0, 0.5]), np.array([2.0, 0.0, 0.75])
    s = gpm.shard_kernel_check("sigma", prior=prior, q=q, m=3, sigma=sentinels(3))
    assert np.isnan(s[0]) and s[1] == 2.0 and np.isnan(s[2])
    assert bits(s)[0] != bits(sentinels(1))[0], "sigma[0] was not written"
    print("RATIO sigma m%d %.4f" % (m, worst))
