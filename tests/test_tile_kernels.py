"""The tile kernels and the diagonal-block kernels in isolation (run with -m gpu on the MI355X box).

Everything goes through the PRODUCT launchers (launch_gemm_nt for fp64 and fp32, launch_diag_syrk_f64[_tiles],
launch_diag256[_ld512], launch_diag256_inv_only[_ld512]) via the hooks of include/gogp_testhooks.h, which copy whole
host arrays to the device and back: every element a launch must leave alone is seen as well as those it writes.

Three kinds of reference:
- exact: operands m / 2^20 (|m| < 2^20) make every product exact in fp64 and every partial sum too (asserted below
  2^53 units), so any summation order gives the same fp64 result -- bit equality catches wrong indexing AND any
  precision loss of the fp64 kernel (these values are not exact in fp32);
- a rounding bound for the fp32 kernel: random full-mantissa operands against fp64,
  |C - C_ref| <= (K + 4) 2^-24 (|alpha| |A||B|^T + |beta C|) -- a bf16 / tf32 path misses it by orders of magnitude;
- sentinels: every element the launch must not write holds a NaN with a payload (or a marked value) and must come back
  bit for bit; tiles computed with beta = 0 are filled with NaN and must come back finite and exact.  Tiles a launch
  skips although it WOULD read them (beta != 0) hold finite values: a NaN read as beta C keeps its payload through
  the accumulation and would come back unchanged from a tile computed by mistake.

The reference model below mirrors the launcher's choice of instance (64-tile 4-wave, 128-tile 4-wave, 128-tile
8-wave) because several semantics are defined per workgroup tile (LOWER's diagonal tiles, the rule filter inside a
diagonal distribution block, the K ranges of ktri / krag0).
"""
import numpy as np
import pytest

from cases import NAN32, NAN64
from cases import tile_instance as instance  # gemm_plan.h

pytestmark = pytest.mark.gpu

T = 128


@pytest.fixture(scope="module")
def gpm():
    from gogp_amd import gp
    return gp


def nan_of(dt):
    return NAN64 if dt == np.float64 else NAN32


def dyadic(rng, shape, bits=20):
    return rng.integers(-(2 ** bits) + 1, 2 ** bits, size=shape).astype(np.float64) / 2.0 ** bits


def view(flat, off, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(rows, cols), strides=(ld * flat.itemsize, flat.itemsize))


def reference(mode, mt, nt, K, alpha, beta, A, B, C, W, BT, bound=None, ktri=0, krag0=-1, new_row0=-1, kbeg0=0,
              rule=0, tpb_shift=0, rblk0=0, cblk0=0, pr=0, Pr=1, pc=0, Pc=1, beta0=-1, **_):
    """Writes into W (float64 view of the expected C) the tiles the launch computes, from A, B, C (float64 views).
    bound (optional, float64 view): |alpha| |A||B|^T + |beta C| over the same K ranges."""
    trap = mode == "TRAP"
    tri = mode in ("LOWER", "LAUUM")
    f = T // BT
    s = tpb_shift + (f == 2)
    k0 = krag0 * f if (krag0 >= 0 and mode in ("RECT", "LOWER") and not ktri) else None
    for ti in range(mt * f):
        for tj in range(ti + 1 if tri else nt * f):
            if trap and (tj * BT) // 256 > (ti * BT) // 256:
                continue
            b = beta
            if rule:
                gI = (rblk0 + (ti >> s)) * Pr + pr
                gJ = (cblk0 + (tj >> s)) * Pc + pc
                msk = (1 << s) - 1
                if gI < gJ or (gI == gJ and (ti & msk) < (tj & msk)):
                    continue
                if rule == 2:
                    b = 0.0 if gI == beta0 else 1.0
            if mode == "LOWER" and new_row0 >= 0 and ti >= new_row0 * f:
                b = 0.0
            kb, ke = 0, K
            if mode == "RECT" and ktri:
                ke = min(K, (tj + 1) * BT)
            if k0 is not None and ti > k0:
                kb = (ti - k0) * BT
            if mode == "LAUUM":
                kb = ti * BT
                if kb < kbeg0:
                    kb, b = kbeg0, 1.0
                if ke <= kb:
                    continue
            r, c = slice(ti * BT, (ti + 1) * BT), slice(tj * BT, (tj + 1) * BT)
            W[r, c] = alpha * (A[r, kb:ke] @ B[c, kb:ke].T)
            if b != 0.0:
                W[r, c] += b * C[r, c]
            if bound is not None:
                bound[r, c] = abs(alpha) * (np.abs(A[r, kb:ke]) @ np.abs(B[c, kb:ke]).T)
                if b != 0.0:
                    bound[r, c] += abs(b * C[r, c])


class Case:
    """Operands of one launch (k candidates) in flat arrays, NaN sentinels everywhere the launch must not read or
    write.  batch: A, B and C share one arena per candidate (the product's layout), bstride elements apart."""

    def __init__(self, prec, mode, mt, nt, K, rng, k=1, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=0,
                 data="dyadic", cfill="data", arena=False):
        self.dt = np.float64 if prec == 64 else np.float32
        self.prec, self.mode, self.mt, self.nt, self.K, self.k = prec, mode, mt, nt, K, k
        nb = mt if mode in ("LOWER", "LAUUM") else nt
        self.M, self.N, self.NB = mt * T, nt * T, nb * T
        self.lda, self.ldb, self.ldc = lda or K, ldb or K, ldc or self.N
        al = 16 // np.dtype(self.dt).itemsize
        sent = nan_of(self.dt)
        ca = (self.M - 1) * self.lda + K
        cb = (self.NB - 1) * self.ldb + K
        cc = (self.M - 1) * self.ldc + self.N
        rnd = lambda n: -(-n // al) * al  # noqa: E731
        if arena:  # [C | gap | A | gap | B | gap] per candidate
            self.c_off = c_off
            self.a_off = rnd(c_off + cc + 2 * al)
            self.b_off = rnd(self.a_off + ca + 2 * al)
            self.bstride = rnd(self.b_off + cb + 3 * al)
            n = self.bstride * k + 4 * al
            self.C = np.full(n, sent, self.dt)
            self.A = self.B = self.C
        else:
            self.a_off, self.b_off, self.c_off = a_off, b_off, c_off
            self.bstride = 0
            if k > 1:
                raise ValueError("a batch lives in an arena")
            self.A = np.full(a_off + ca + 3 * al, sent, self.dt)
            self.B = np.full(b_off + cb + 5 * al, sent, self.dt)
            self.C = np.full(c_off + cc + 7 * al, sent, self.dt)
        for c in range(k):
            for v in (self.a(c), self.b(c)):
                if data == "dyadic":
                    v[:] = dyadic(rng, v.shape)
                else:
                    v[:] = rng.standard_normal(v.shape)
            if cfill == "data":
                cv = self.c(c)
                cv[:] = dyadic(rng, cv.shape, 40) * 16 if data == "dyadic" else rng.standard_normal(cv.shape)
            elif cfill == "nan":
                self.c(c)[:] = sent

    def a(self, c=0, arr=None):
        return view(self.A if arr is None else arr, self.a_off + c * self.bstride, self.M, self.K, self.lda)

    def b(self, c=0, arr=None):
        return view(self.B if arr is None else arr, self.b_off + c * self.bstride, self.NB, self.K, self.ldb)

    def c(self, c=0, arr=None):
        return view(self.C if arr is None else arr, self.c_off + c * self.bstride, self.M, self.N, self.ldc)

    def run(self, gpm, alpha=-1.0, beta=1.0, **opts):
        if self.k > 1:
            opts = dict(opts, k=self.k, bstride=self.bstride)
        return gpm.gemm_nt_check(self.mode, self.mt, self.nt, self.K, self.A, self.B, self.C, alpha, beta,
                                 lda=self.lda, ldb=self.ldb, ldc=self.ldc, a_off=self.a_off, b_off=self.b_off,
                                 c_off=self.c_off, **opts)

    def expect(self, alpha=-1.0, beta=1.0, small_below=384, with_bound=False, **opts):
        """Expected C (float64, flat) and, with_bound, the elementwise rounding budget (0 where nothing is computed)."""
        BT, _ = instance(self.prec, self.mode, self.mt, self.nt, self.k, small_below)
        want = self.C.astype(np.float64)
        bound = np.zeros_like(want) if with_bound else None
        for c in range(self.k):
            A = self.a(c).astype(np.float64)
            B = self.b(c).astype(np.float64)
            C = self.c(c).astype(np.float64)
            if self.prec == 64 and not with_bound:  # exactness precondition: every partial sum below 2^53 units
                mag = np.abs(A).max() * np.abs(B).max() * self.K + abs(beta) * np.nan_to_num(np.abs(C)).max()
                assert mag < 2.0 ** 13, mag
            reference(self.mode, self.mt, self.nt, self.K, alpha, beta, A, B, C, self.c(c, want), BT,
                      None if bound is None else self.c(c, bound), **opts)
        return want, bound


def check(got, want, before, bound=None, u=None, chunk=1 << 22):
    """Sentinels (NaN in want) bit for bit as they were; everything else exact, or within bound * u.  In chunks: the
    8-wave cases hold a few hundred MB per array."""
    ut = np.uint64 if got.dtype == np.float64 else np.uint32
    gbits, bbits = got.view(ut), before.view(ut)
    for s0 in range(0, want.size, chunk):
        sl = slice(s0, s0 + chunk)
        w = want[sl]
        nan = np.isnan(w)
        bad = np.flatnonzero(gbits[sl][nan] != bbits[sl][nan])
        assert bad.size == 0, "%d sentinels changed, first at %d" % (bad.size, s0 + np.flatnonzero(nan)[bad[0]])
        g, w = got[sl][~nan].astype(np.float64), w[~nan]
        if bound is None:
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, "%d of %d elements differ, first at %d: %r vs %r" % (
                bad.size, w.size, s0 + np.flatnonzero(~nan)[bad[0]], g[bad[0]], w[bad[0]])
        else:
            err = np.abs(g - w)
            lim = bound[sl][~nan] * u
            bad = np.flatnonzero(~(err <= lim))
            assert bad.size == 0, "%d of %d elements outside the bound, first at %d, worst ratio %g" % (
                bad.size, w.size, s0 + np.flatnonzero(~nan)[bad[0]], np.nanmax(err / np.maximum(lim, 1e-300)))


def run_check(gpm, case, alpha=-1.0, beta=1.0, **opts):
    got = case.run(gpm, alpha, beta, **opts)
    if case.prec == 64:
        want, _ = case.expect(alpha, beta, **opts)
        check(got, want, case.C)
    else:
        want, bound = case.expect(alpha, beta, with_bound=True, **opts)
        check(got, want, case.C, bound, (case.K + 4) * 2.0 ** -24)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# every compiled instance, at shapes picked from the launcher's rules
# ---------------------------------------------------------------------------------------------------------------------
# (precision, mode, mt, nt, K, k, small_below, instance, the rule the shape hits)
INSTANCES = [
    (64, "RECT", 3, 5, 16, 1, 384, (64, 4), "15 tiles < 384, one K-step"),
    (64, "RECT", 7, 11, 1040, 1, 384, (64, 4), "77 tiles, K >= 1024 and not a multiple of 128"),
    (64, "RECT", 24, 24, 32, 1, 384, (64, 4), "576 tiles in 513..768"),
    (64, "RECT", 19, 27, 48, 1, 384, (64, 4), "513 tiles: the first of 513..768"),
    (64, "RECT", 16, 32, 16, 1, 384, (128, 4), "512 tiles: the last below 513"),
    (64, "RECT", 20, 20, 80, 1, 384, (128, 4), "400 tiles"),
    (64, "RECT", 30, 30, 16, 1, 384, (128, 4), "900 tiles = 4 mod 8"),
    (64, "RECT", 17, 23, 1040, 1, 384, (128, 4), "391 tiles = 7 mod 8, K >= 1024"),
    (64, "RECT", 13, 31, 32, 1, 384, (128, 4), "403 tiles = 3 mod 8"),
    (64, "RECT", 5, 77, 16, 1, 384, (128, 4), "385 tiles = 1 mod 8"),
    (64, "RECT", 3, 5, 48, 1, 10, (128, 4), "small_below lowered: 15 tiles = 7 mod 8 on 128-tiles"),
    (64, "RECT", 20, 20, 48, 1, 1000, (64, 4), "small_below raised: 400 tiles on 64-tiles"),
    (64, "RECT", 64, 48, 16, 1, 384, (128, 8), "3072 tiles"),
    (64, "LOWER", 27, 27, 16, 1, 384, (64, 4), "378 tiles < 384"),
    (64, "LOWER", 28, 28, 64, 1, 384, (128, 4), "406 tiles = 6 mod 8"),
    (64, "LOWER", 32, 32, 32, 1, 384, (64, 4), "528 tiles in 513..768"),
    (64, "LOWER", 39, 39, 16, 1, 384, (128, 4), "780 tiles = 4 mod 8"),
    (64, "LOWER", 41, 41, 1040, 1, 384, (128, 4), "861 tiles = 5 mod 8, K >= 1024"),
    (64, "LOWER", 28, 28, 16, 8, 384, (128, 8), "8 candidates x 406 tiles = 3248"),
    (64, "LAUUM", 5, 5, 640, 1, 384, (128, 8), "LAUUM: always 128 x 8"),
    (64, "LAUUM", 3, 3, 400, 1, 384, (128, 8), "LAUUM, K not a multiple of 128"),
    (32, "RECT", 3, 5, 32, 1, 384, (64, 4), "15 tiles < 384, one K-step"),
    (32, "RECT", 7, 11, 1056, 1, 384, (64, 4), "77 tiles, K >= 1024 and not a multiple of 128"),
    (32, "RECT", 24, 24, 64, 1, 384, (128, 4), "576 tiles: no 513..768 rule in fp32"),
    (32, "RECT", 17, 23, 32, 1, 384, (128, 4), "391 tiles = 7 mod 8"),
    (32, "RECT", 3, 5, 96, 1, 10, (128, 4), "small_below lowered"),
    (32, "RECT", 20, 20, 32, 1, 1000, (64, 4), "small_below raised"),
    (32, "RECT", 64, 48, 32, 1, 384, (128, 8), "3072 tiles"),
    (32, "LOWER", 27, 27, 32, 1, 384, (64, 4), "378 tiles < 384"),
    (32, "LOWER", 32, 32, 1056, 1, 384, (128, 4), "528 tiles: 128 x 4 in fp32, K >= 1024"),
    (32, "LOWER", 78, 78, 32, 1, 384, (128, 8), "3081 tiles = 1 mod 8"),
    (32, "LAUUM", 5, 5, 640, 1, 384, (128, 8), "LAUUM: always 128 x 8"),
]


def test_instance_table_covers_all_14():
    seen = {(p, "LAUUM" if m == "LAUUM" else ("RECT" if m in ("RECT", "TRAP") else "LOWER"), inst)
            for p, m, mt, nt, K, k, sb, inst, _ in INSTANCES}
    assert len(seen) == 14, sorted(seen)
    for p, m, mt, nt, K, k, sb, inst, why in INSTANCES:
        assert instance(p, m, mt, nt, k, sb) == inst, why


@pytest.mark.parametrize("prec,mode,mt,nt,K,k,small_below,inst,why", INSTANCES,
                         ids=["%d-%s-%dx%d-K%d-k%d-sb%d" % c[:7] for c in INSTANCES])
def test_instance(gpm, prec, mode, mt, nt, K, k, small_below, inst, why):
    rng = np.random.default_rng(mt * 1000 + nt * 10 + K + prec)
    case = Case(prec, mode, mt, nt, K, rng, k=k, arena=k > 1, data="dyadic" if prec == 64 else "normal")
    run_check(gpm, case, -1.0, 1.0, small_below=small_below)


# ---------------------------------------------------------------------------------------------------------------------
# leading dimensions, offsets, alpha / beta
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mode,mt,nt,small_below", [("RECT", 3, 4, 384), ("RECT", 3, 4, 1), ("LOWER", 4, 4, 384),
                                                    ("LOWER", 4, 4, 1), ("LAUUM", 4, 4, 384), ("TRAP", 4, 6, 384),
                                                    ("TRAP", 4, 6, 1)])
def test_leading_dims_and_offsets(gpm, prec, mode, mt, nt, small_below):
    rng = np.random.default_rng(7 + mt + nt + small_below)
    K = 4 * T + (32 if prec == 32 else 48)
    al = 2 if prec == 64 else 4
    N = nt * T
    ldc = N + 24 * al
    case = Case(prec, mode, mt, nt, K, rng, lda=K + 8 * al, ldb=K + 20 * al, ldc=ldc, a_off=3 * al, b_off=5 * al,
                c_off=2 * ldc + 6 * al, data="dyadic" if prec == 64 else "normal")
    run_check(gpm, case, -1.0, 1.0, small_below=small_below)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (-1.0, 1.0)])
@pytest.mark.parametrize("mode", ["RECT", "LOWER", "LAUUM"])
def test_alpha_beta_product_values(gpm, prec, alpha, beta, mode):
    rng = np.random.default_rng(11)
    case = Case(prec, mode, 3, 3, 3 * T + 64, rng, cfill="nan" if beta == 0.0 else "data",
                data="dyadic" if prec == 64 else "normal")
    run_check(gpm, case, alpha, beta)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("small_below", [384, 1])
def test_alpha_beta_nontrivial(gpm, prec, small_below):
    """alpha = 0.3, beta = -1.7: the kernels start the accumulators at fl(beta / alpha) C and scale by alpha at the
    end -- two extra roundings, within (K + 4) u (|alpha| |A||B|^T + |beta C|)."""
    rng = np.random.default_rng(13)
    K = 2 * T + 32
    case = Case(prec, "RECT", 2, 3, K, rng, data="normal")
    got = case.run(gpm, 0.3, -1.7, small_below=small_below)
    want, bound = case.expect(0.3, -1.7, small_below=small_below, with_bound=True)
    check(got, want, case.C, bound, (K + 4) * (2.0 ** -53 if prec == 64 else 2.0 ** -24))


# ---------------------------------------------------------------------------------------------------------------------
# mode semantics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
def test_lauum_skips_columns_left_of_the_tile_row(gpm, prec):
    """LAUUM tile (ti, tj) sums k in [ti * 128, K); the columns left of that hold NONZERO data, which must not count."""
    rng = np.random.default_rng(17)
    case = Case(prec, "LAUUM", 5, 5, 5 * T, rng, data="dyadic" if prec == 64 else "normal", cfill="nan")
    a = case.a()
    for i in range(1, 5):  # the skipped columns are really there
        assert np.count_nonzero(a[i * T:, :i * T]) > 0.9 * a[i * T:, :i * T].size
    run_check(gpm, case, 1.0, 0.0)


@pytest.mark.parametrize("kbeg0", [256, 208])
def test_lauum_kbeg0_accumulates_above_and_overwrites_below(gpm, kbeg0):
    """The second launch of the two-launch K^-1: tile rows with ti * 128 < kbeg0 ACCUMULATE the sum over
    [kbeg0, K) into C (beta = 1 whatever the launch's beta); the rows below use the launch's beta (0: NaN-filled)."""
    rng = np.random.default_rng(19)
    case = Case(64, "LAUUM", 5, 5, 5 * T, rng)
    c = case.c()
    c[-(-kbeg0 // T) * T:, :] = NAN64
    got = case.run(gpm, 1.0, 0.0, kbeg0=kbeg0)
    want, _ = case.expect(1.0, 0.0, kbeg0=kbeg0)
    check(got, want, case.C)


@pytest.mark.parametrize("kbeg0", [256, 384, 208])
def test_lauum_two_launches_equal_one(gpm, kbeg0):
    """LAUUM in two launches (K = kbeg0, then the rest with kbeg0) equals the one-launch form bit for bit on random
    full-mantissa data: the same products in the same order."""
    rng = np.random.default_rng(23)
    K = 5 * T
    case = Case(64, "LAUUM", 5, 5, K, rng, data="normal", cfill="nan")
    one = case.run(gpm, 1.0, 0.0)
    half = gpm.gemm_nt_check("LAUUM", 5, 5, kbeg0, case.A, case.B, case.C, 1.0, 0.0, lda=K, ldb=K, ldc=case.ldc)
    two = gpm.gemm_nt_check("LAUUM", 5, 5, K, case.A, case.B, half, 1.0, 0.0, lda=K, ldb=K, ldc=case.ldc, kbeg0=kbeg0)
    np.testing.assert_array_equal(two.view(np.uint64), one.view(np.uint64))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mt,small_below", [(3, 384), (3, 1), (200, 384)])
def test_ktri(gpm, prec, mt, small_below):
    """ktri: B (nt*128 x K) lower triangular -- tile column tj sums k < (tj + 1) * tile.  With a lower-triangular B
    the result is the full product on every instance; with a dense B it is the sum over exactly that K range."""
    rng = np.random.default_rng(29 + mt)
    K = 2 * T
    data = "dyadic" if prec == 64 else "normal"
    case = Case(prec, "RECT", mt, 2, K, rng, data=data)
    run_check(gpm, case, -1.0, 1.0, ktri=1, small_below=small_below)  # dense B: the K range itself
    b = case.b()
    b[:] = np.tril(b)
    got = case.run(gpm, -1.0, 1.0, ktri=1, small_below=small_below)
    want, bound = case.expect(-1.0, 1.0, small_below=small_below, with_bound=prec == 32)  # no ktri: full product
    check(got, want, case.C, bound, (K + 4) * 2.0 ** -24)


def krag0_pattern(a, krag0, kind):
    """Zero A (rows from krag0 * 128 on) left of its K start: 'elementwise' row krag0*128 + r for k < r;
    'doc' (common.h) row krag0*128 + r for k < 64 * floor(r / 64); 'blocks128' row block krag0 + i for k < 128 i."""
    for r in range(a.shape[0] - krag0 * T):
        z = {"elementwise": r, "doc": 64 * (r // 64), "blocks128": T * (r // T)}[kind]
        a[krag0 * T + r, :z] = 0


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mode,mt,nt,krag0", [("RECT", 6, 3, 2), ("RECT", 5, 2, 0), ("LOWER", 4, 4, 1)])
@pytest.mark.parametrize("small_below", [384, 1])
def test_krag0(gpm, prec, mode, mt, nt, krag0, small_below):
    """krag0: tile row ti > krag0 starts at k = (ti - krag0) * tile, in units of the
    launch's OWN tile -- the 64-tile launches also skip k in [128 i, 128 i + 64) for rows 64..127 of block krag0 + i.
    Dense data pins the K range exactly; A zeroed to the precondition common.h states (per 64-row half) and to Y's
    elementwise pattern gives the full product on both tile sizes; zeroed only per 128-row block it does not on 64."""
    rng = np.random.default_rng(31 + mt + small_below)
    K = (mt - krag0) * T
    data = "dyadic" if prec == 64 else "normal"
    case = Case(prec, mode, mt, nt, K, rng, data=data)
    run_check(gpm, case, -1.0, 1.0, krag0=krag0, small_below=small_below)  # dense: the K ranges themselves
    BT, _ = instance(prec, mode, mt, nt, 1, small_below)
    a = case.a()
    saved = a.copy()
    for kind in ("elementwise", "doc", "blocks128"):
        a[:] = saved
        krag0_pattern(a, krag0, kind)
        got = case.run(gpm, -1.0, 1.0, krag0=krag0, small_below=small_below)
        want, bound = case.expect(-1.0, 1.0, small_below=small_below, with_bound=prec == 32)  # the full product
        if kind == "blocks128" and BT == 64 and mt - krag0 > 0:
            with pytest.raises(AssertionError):
                check(got, want, case.C, bound, (K + 4) * 2.0 ** -24)
        else:
            check(got, want, case.C, bound, (K + 4) * 2.0 ** -24)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mt,new_row0,small_below", [(6, 3, 384), (6, 3, 1), (6, 0, 384), (28, 20, 384)])
def test_new_row0(gpm, prec, mt, new_row0, small_below):
    """LOWER with new_row0: tile rows >= new_row0 overwrite C (beta = 0: NaN-filled, must come back finite), the rows
    above accumulate with the launch's beta."""
    rng = np.random.default_rng(37 + mt)
    case = Case(prec, "LOWER", mt, mt, 2 * T, rng, data="dyadic" if prec == 64 else "normal")
    case.c()[new_row0 * T:, :] = nan_of(case.dt)
    run_check(gpm, case, -1.0, 1.0, new_row0=new_row0, small_below=small_below)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mt,nt,small_below", [(6, 6, 384), (6, 6, 1), (5, 8, 384), (24, 24, 384)])
def test_trap(gpm, prec, mt, nt, small_below):
    """TRAP: the tiles of strictly upper 256-blocks (counted from the C origin) are skipped.  They hold a marked FINITE
    value, not a NaN: a tile computed with beta != 0 over a NaN carries the NaN's payload through (beta/alpha) C and the
    final alpha scaling and would give back the same bits."""
    rng = np.random.default_rng(41 + mt + nt)
    case = Case(prec, "TRAP", mt, nt, 96 if prec == 64 else 128, rng, data="dyadic" if prec == 64 else "normal")
    c = case.c()
    for bi in range(mt // 2 + 1):
        c[bi * 256:(bi + 1) * 256, (bi + 1) * 256:] = 999.5
    run_check(gpm, case, -1.0, 1.0, small_below=small_below)


RULE_LAUNCHES = []
for _Pr, _Pc in [(1, 2), (2, 2), (2, 4)]:
    for _pr in range(_Pr):
        for _pc in range(_Pc):
            RULE_LAUNCHES.append((_Pr, _Pc, _pr, _pc))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("Pr,Pc,pr,pc", RULE_LAUNCHES)
@pytest.mark.parametrize("small_below", [384, 1])
def test_rule_filter(gpm, prec, Pr, Pc, pr, pc, small_below):
    """The sharded tile filter on the block maps of 1x2, 2x2 and 2x4 grids: rule 1 keeps the tiles of the GLOBAL lower
    triangle; rule 2 also overwrites the blocks of global row block beta0 (NaN-filled) and accumulates elsewhere."""
    rng = np.random.default_rng(43 + 8 * Pr + 4 * Pc + 2 * pr + pc)
    mt, nt, s, rblk0, cblk0 = 4, 6, 1, 1, 0  # 2 x 3 local distribution blocks of 2 x 2 tiles
    data = "dyadic" if prec == 64 else "normal"
    grid = dict(tpb_shift=s, rblk0=rblk0, cblk0=cblk0, pr=pr, Pr=Pr, pc=pc, Pc=Pc, small_below=small_below)
    case = Case(prec, "RECT", mt, nt, 64 if prec == 64 else 96, rng, data=data)
    run_check(gpm, case, -1.0, 1.0, rule=1, **grid)
    beta0 = (rblk0 + 1) * Pr + pr  # the second local row block
    case.c()[2 * T:4 * T, :] = nan_of(case.dt)
    run_check(gpm, case, -1.0, 1.0, rule=2, beta0=beta0, **grid)


@pytest.mark.parametrize("mode,mt,nt,k", [("RECT", 3, 2, 3), ("LOWER", 3, 3, 3), ("RECT", 20, 20, 8),
                                          ("LAUUM", 3, 3, 8)])
def test_candidate_batch(gpm, mode, mt, nt, k):
    """k candidates on gridDim.z, A / B / C of candidate c bstride elements after candidate 0's (one arena slot
    each), different data per slot; the gaps between slots keep their sentinels."""
    rng = np.random.default_rng(47 + k)
    case = Case(64, mode, mt, nt, 2 * T + 16, rng, k=k, arena=True)
    run_check(gpm, case, -1.0, 1.0)


@pytest.mark.parametrize("small_below", [384, 1])
def test_sgemm_fragment_layout_asymmetric(gpm, small_below):
    """A = I against an asymmetric integer B catches a transposed C/D fragment map of v_mfma_f32_32x32x2_f32
    (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))."""
    A = np.eye(T, dtype=np.float32)
    B = np.arange(T * T, dtype=np.float32).reshape(T, T)
    got = gpm.gemm_nt_check("RECT", 1, 1, T, A, B, np.full((T, T), NAN32, np.float32), 1.0, 0.0,
                            small_below=small_below)
    np.testing.assert_array_equal(got, B.T)


# ---------------------------------------------------------------------------------------------------------------------
# diagsyrk.hip: the fp32 path's fp64 update of the diagonal blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,nblocks,K,row_stride_rows", [(256, 1, 16, None), (256, 3, 48, None), (256, 2, 272, None),
                                                          (512, 1, 16, 512), (512, 3, 64, 600)])
def test_diag_syrk_sums_in_fp64(gpm, bs, nblocks, K, row_stride_rows):
    """Floats m / 2^12 (|m| < 2^12): products and sums are exact in fp64, not in fp32 -- bit equality pins "summed in
    fp64".  Only the lower 64-tiles of each block change; the upper ones and the blocks past nblocks keep their
    sentinels, and the floats outside the rows / K range are NaN (never read)."""
    rng = np.random.default_rng(53 + bs + K)
    ld = K + 20
    l_off = 8
    stride = (row_stride_rows or bs) * ld
    nL = l_off + (nblocks - 1) * stride + (bs - 1) * ld + K + 12
    L = np.full(nL, NAN32, np.float32)
    rows = []
    for b in range(nblocks):
        v = view(L, l_off + b * stride, bs, K, ld)
        v[:] = dyadic(rng, (bs, K), 12)
        rows.append(v.astype(np.float64))
    D = np.full((nblocks + 1) * bs * bs, NAN64)
    blocks = D.reshape(nblocks + 1, bs, bs)
    for b in range(nblocks):
        blocks[b] = dyadic(rng, (bs, bs), 24) * 64
    got = gpm.diag_syrk_check(L, D, K, nblocks, bs=bs, ld=ld, l_off=l_off,
                              row_stride=stride if bs == 512 else None)
    want = D.copy().reshape(nblocks + 1, bs, bs)
    for b in range(nblocks):
        upd = blocks[b] - rows[b] @ rows[b].T
        for ti in range(bs // 64):
            for tj in range(ti + 1):
                r, c = slice(ti * 64, ti * 64 + 64), slice(tj * 64, tj * 64 + 64)
                want[b][r, c] = upd[r, c]
    check(got, want.ravel(), D)
    # the same sums in fp32 are not exact: the test would see a float accumulation
    r32 = rows[0].astype(np.float32)
    assert not np.array_equal((r32 @ r32.T).astype(np.float64), rows[0] @ rows[0].T)


# ---------------------------------------------------------------------------------------------------------------------
# diag256.hip: the product build of the diagonal-block factor + inverse
# ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def spd(rng, cond, n=256):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0, -np.log10(cond), n)
    A = (Q * lam) @ Q.T
    return (A + A.T) / 2


def residuals(A, L, X):
    Al, Ll, Xl = (np.asarray(m, dtype=np.longdouble) for m in (A, L, X))
    back = np.linalg.norm((Al - Ll @ Ll.T).astype(np.float64)) / np.linalg.norm(A)
    inv = np.linalg.norm((Ll @ Xl - np.eye(len(A), dtype=np.longdouble)).astype(np.float64))
    kappa = np.linalg.norm(L) * np.linalg.norm(X)
    return back, inv, kappa


@pytest.mark.parametrize("cond", [1e2, 1e6, 1e9, 1e12])
def test_diag256_accuracy(gpm, cond):
    """Backward error ||A - L L^T|| <= 2 * 256 u ||A|| whatever the condition number; ||L Dinv - I|| <= 2 * 256 u
    kappa(L); upper triangles zero-filled.  The strictly upper triangle of A is NaN: only the lower one is read."""
    rng = np.random.default_rng(int(np.log10(cond)))
    A = spd(rng, cond)
    An = A.copy()
    An[np.triu_indices(256, 1)] = np.nan
    L, X, info = gpm.diag256_product(An, 0, row0=0, nvalid=256)
    assert info == 0
    assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(X, 1) == 0)
    back, inv, kappa = residuals(A, L, X)
    assert back <= 2 * 256 * U, back
    assert inv <= 2 * 256 * U * kappa, (inv, kappa)


@pytest.mark.parametrize("nv", [1, 64, 188, 256])
def test_diag256_padded_block(gpm, nv):
    """A block with nv valid rows (global rows row0 .. row0 + nv - 1 < nvalid) and the identity padding the product
    puts below n: the factor / inverse of the valid part and the identity."""
    rng = np.random.default_rng(59 + nv)
    A = np.eye(256)
    A[:nv, :nv] = spd(rng, 1e4, nv) if nv > 1 else 2.0
    row0 = 512
    L, X, info = gpm.diag256_product(A, 0, row0=row0, nvalid=row0 + nv)
    assert info == 0
    back, inv, kappa = residuals(A, L, X)
    assert back <= 2 * 256 * U and inv <= 2 * 256 * U * kappa, (back, inv, kappa)
    np.testing.assert_allclose(L[nv:, nv:], np.eye(256 - nv), rtol=0, atol=4 * U)
    np.testing.assert_array_equal(L[nv:, :nv], 0.0)


def notpd(rng, p, how):
    L0 = np.tril(rng.standard_normal((256, 256)) * 0.05, -1) + np.diag(rng.uniform(1, 2, 256))
    A = L0 @ L0.T
    if how == "negative":
        A[p, p] -= L0[p, p] ** 2 + 1.0
    else:  # row / column p zero: pivot p is exactly A[p, p] -- 0 or NaN
        A[p, :] = 0.0
        A[:, p] = 0.0
        A[p, p] = 0.0 if how == "zero" else np.nan
    return A


@pytest.mark.parametrize("p", [0, 15, 16, 127, 128, 255])
@pytest.mark.parametrize("how", ["negative", "zero", "nan"])
def test_diag256_reports_first_failing_pivot(gpm, p, how):
    rng = np.random.default_rng(61 + p)
    A = notpd(rng, p, how)
    row0 = 768
    assert gpm.diag256_product(A, 0, row0=row0, nvalid=row0 + 256)[2] == row0 + p + 1
    assert gpm.diag256_product(A, 1, row0=row0, nvalid=row0 + p + 1)[2] == row0 + p + 1
    # a failing pivot at or after nvalid is not reported
    assert gpm.diag256_product(A, 0, row0=row0, nvalid=row0 + p)[2] == 0
    assert gpm.diag256_product(A, 1, row0=row0, nvalid=row0 + p)[2] == 0


def test_diag256_variants_and_stamped_build(gpm):
    """ld 512 variants equal the ld 256 ones bit for bit (and leave Dinv's other 256 columns alone); the inverse-only
    variants invert the factor to the same accuracy (their 1 / L_jj comes from v_rcp_f64 instead of the factor's
    v_rsq_f64: not the same bits); the stamped diagnostic build (gogp_test_diag256) equals the product build."""
    rng = np.random.default_rng(67)
    A = spd(rng, 1e6)
    L0, X0, i0 = gpm.diag256_product(A, 0)
    sentinel = np.full((256, 512), NAN64)
    L1, X1, i1 = gpm.diag256_product(A, 1, Dinv=sentinel)
    assert i0 == i1 == 0
    np.testing.assert_array_equal(L1.view(np.uint64), L0.view(np.uint64))
    np.testing.assert_array_equal(X1[:, :256].view(np.uint64), X0.view(np.uint64))
    np.testing.assert_array_equal(X1[:, 256:].view(np.uint64), sentinel[:, 256:].view(np.uint64))
    # inverse only, on the factor (A's place holds L; L stays as handed in)
    Lin = np.full((256, 256), NAN64)
    Lr, X2, _ = gpm.diag256_product(L0, 2, L=Lin)
    np.testing.assert_array_equal(Lr.view(np.uint64), Lin.view(np.uint64))
    _, X3, _ = gpm.diag256_product(L0, 3, Dinv=sentinel)
    np.testing.assert_array_equal(X3[:, :256].view(np.uint64), X2.view(np.uint64))
    np.testing.assert_array_equal(X3[:, 256:].view(np.uint64), sentinel[:, 256:].view(np.uint64))
    _, inv, kappa = residuals(A, L0, X2)
    assert inv <= 2 * 256 * U * kappa
    assert np.all(np.triu(X2, 1) == 0)
    np.testing.assert_allclose(X2, X0, rtol=0, atol=2 * 256 * U * kappa * np.abs(X0).max())
    # the stamped build that tools/ measures computes the same bits
    Ls, Xs, _, _ = gpm.diag256_check(A)
    np.testing.assert_array_equal(Ls.view(np.uint64), L0.view(np.uint64))
    np.testing.assert_array_equal(Xs.view(np.uint64), X0.view(np.uint64))
