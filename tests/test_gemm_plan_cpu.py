"""The launch plan of the tile kernels (gogp_amd/csrc/gemm_plan.h) through gogp_test_gemm_plan, which never
touches the device.  The expectation is a model written here, never the library: the instance rule is
cases.tile_instance (the one tests/test_tile_kernels.py builds its references on), the grid follows from the tile
enumeration of that instance, and the flops are counted tile by tile from the K range each 128-tile sums
(2 * 128 * 128 * len(K range), the tiles the kernel skips not counted; a diagonal tile of LOWER / LAUUM counts whole).
Every count is an integer below 2^53 (times a power of two), so the comparison is exact.

TRAP: the launcher books a closed form that equals the tile count for an even number of tile columns and
mt >= nt - 2 -- every trapezoid the factorisation launches (api.hip) -- so the cases stay inside that."""
import ctypes

import pytest

from cases import tile_instance
from gogp_amd import _lib

T = 128
MODES = {"RECT": 0, "LOWER": 1, "LAUUM": 2, "TRAP": 3}


@pytest.fixture(scope="module")
def hk():
    _lib.build()
    return _lib.hooks()


def plan(hk, prec, mode, mt, nt, K, **opts):
    out = _lib.CGemmPlan()
    o = _lib.CGemmOpts(**dict(_lib.CGemmOpts.DEFAULTS, **opts))
    rc = hk.gogp_test_gemm_plan(prec, MODES[mode], mt, nt, K, ctypes.byref(o), ctypes.byref(out))
    assert rc == _lib.GOGP_OK, rc
    return (out.tile, out.waves), out.grid_x, out.grid_z, out.flops, out.tag


def model(prec, mode, mt, nt, K, k=1, small_below=384, ktri=0, krag0=-1, kbeg0=0, rule=0, tpb_shift=0, rblk0=0,
          cblk0=0, pr=0, Pr=1, pc=0, Pc=1, **_):
    tri = mode in ("LOWER", "LAUUM")
    tile, waves = tile_instance(prec, mode, mt, nt, k, small_below)
    f = T // tile
    if tri:
        gx = mt * f * (mt * f + 1) // 2
    elif rule:
        gx = 8 * -(-mt * f // 8) * nt * f
    else:
        gx = mt * f * nt * f
    flops = 0
    for ti in range(mt):
        for tj in range(ti + 1 if tri else nt):
            if mode == "TRAP" and tj // 2 > ti // 2:
                continue
            if rule:  # a distribution block is 2^tpb_shift 128-tiles; inside a diagonal block the lower tiles
                gI = (rblk0 + (ti >> tpb_shift)) * Pr + pr
                gJ = (cblk0 + (tj >> tpb_shift)) * Pc + pc
                msk = (1 << tpb_shift) - 1
                if gI < gJ or (gI == gJ and (ti & msk) < (tj & msk)):
                    continue
            kb, ke = 0, K
            if mode == "RECT" and ktri:
                ke = min(K, (tj + 1) * T)
            if mode in ("RECT", "LOWER") and krag0 >= 0 and not ktri:
                kb = max(0, ti - krag0) * T
            if mode == "LAUUM":
                kb = max(ti * T, kbeg0)
            flops += 2 * T * T * max(0, ke - kb)
    ntiles = mt * (mt + 1) // 2 if tri else mt * nt
    tag = (0 if mode == "TRAP" else MODES[mode]) * 10 ** 8 + (K // 16) * 10 ** 5 + min(ntiles, 99999)
    return (tile, waves), gx, k, float(flops * k), tag


def agree(hk, prec, mode, mt, nt, K, **opts):
    got, want = plan(hk, prec, mode, mt, nt, K, **opts), model(prec, mode, mt, nt, K, **opts)
    assert got == want, (prec, mode, mt, nt, K, opts, got, want)
    return got


# (tiles, fp64 instance, fp32 instance): only fp64 has the 513..768 band
BAND_EDGES = [(383, (64, 4), (64, 4)), (384, (128, 4), (128, 4)), (512, (128, 4), (128, 4)), (513, (64, 4), (128, 4)),
              (768, (64, 4), (128, 4)), (769, (128, 4), (128, 4)), (3071, (128, 4), (128, 4)),
              (3072, (128, 8), (128, 8))]


@pytest.mark.parametrize("tiles,inst64,inst32", BAND_EDGES)
def test_band_edges_rect(hk, tiles, inst64, inst32):
    for mt, nt in ((1, tiles), (tiles, 1)):
        assert agree(hk, 64, "RECT", mt, nt, 64)[0] == inst64
        assert agree(hk, 32, "RECT", mt, nt, 64)[0] == inst32


@pytest.mark.parametrize("k,mt,nt,inst", [(3, 1, 127, (64, 4)), (3, 1, 128, (128, 4)), (3, 1, 171, (64, 4)),
                                          (3, 1, 256, (64, 4)), (3, 1, 257, (128, 4)), (8, 1, 383, (128, 4)),
                                          (8, 1, 384, (128, 8)), (8, 8, 8, (128, 4)), (8, 5, 13, (64, 4)), (8, 8, 12, (64, 4)),
                                          (8, 1, 47, (64, 4)), (8, 1, 48, (128, 4)), (3, 16, 8, (128, 4)),
                                          (8, 16, 24, (128, 8))])
def test_candidate_batch_counts_all_candidates(hk, k, mt, nt, inst):
    """The same edges reached through the batch: k = 3 with 128 tiles (384) and k = 8 with 384 (3072) among them."""
    got = agree(hk, 64, "RECT", mt, nt, 32, k=k, bstride=1 << 24)
    assert got[0] == inst and got[2] == k


@pytest.mark.parametrize("prec", [64, 32])
def test_lower(hk, prec):
    assert agree(hk, prec, "LOWER", 27, 27, 64)[0] == (64, 4)  # 378 tiles
    assert agree(hk, prec, "LOWER", 28, 28, 64)[0] == (128, 4)  # 406 tiles
    assert agree(hk, prec, "LOWER", 32, 32, 64)[0] == ((64, 4) if prec == 64 else (128, 4))  # 528 tiles
    assert agree(hk, prec, "LOWER", 78, 78, 64)[0] == (128, 8)  # 3081 tiles


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mt", [1, 4, 27, 36, 80])
def test_lauum_is_always_128x8(hk, prec, mt):
    assert agree(hk, prec, "LAUUM", mt, mt, mt * T)[0] == (128, 8)
    assert agree(hk, prec, "LAUUM", mt, mt, mt * T, small_below=1 << 20)[0] == (128, 8)


def test_lauum_kbeg0_flops(hk):
    """The second of two launches sums k >= max(ti * 128, 256): 2 * 128^2 * (1 * 256 + 2 * 256 + 3 * 256 + 4 * 128)."""
    got = agree(hk, 64, "LAUUM", 4, 4, 512, kbeg0=256)
    assert got[3] == 2.0 * T * T * (256 + 2 * 256 + 3 * 256 + 4 * 128)
    assert agree(hk, 64, "LAUUM", 4, 4, 512)[3] == 2.0 * T * T * (512 + 2 * 384 + 3 * 256 + 4 * 128)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("tiles", [1, 383, 384, 512, 513, 600, 768, 769, 3071, 3072, 4000])
def test_small_below_override(hk, prec, tiles):
    """small_below = 1: nothing is small but the fp64 band, which does not look at small_below; a large small_below
    makes everything small, the >= 3072 launches included."""
    low = agree(hk, prec, "RECT", 1, tiles, 32, small_below=1)[0]
    band = prec == 64 and 513 <= tiles <= 768
    assert low == ((64, 4) if band else (128, 8) if tiles >= 3072 else (128, 4))
    assert agree(hk, prec, "RECT", 1, tiles, 32, small_below=1 << 20)[0] == (64, 4)
    assert agree(hk, prec, "LOWER", 30, 30, 32, small_below=1)[0] == (128, 4)  # 465 tiles
    assert agree(hk, prec, "LOWER", 30, 30, 32, small_below=466)[0] == (64, 4)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("small_below", [384, 1])
@pytest.mark.parametrize("mt,nt", [(4, 6), (9, 3), (8, 2), (17, 1)])
def test_rule_launch_grid(hk, prec, small_below, mt, nt):
    """A filtered launch deals the tile ROWS to the 8 XCD groups: 8 * ceil(mt / 8) * nt workgroups, in tiles of the
    launched instance."""
    f = 2 if small_below == 384 else 1
    for rule in (1, 2):
        got = agree(hk, prec, "RECT", mt, nt, 64, rule=rule, small_below=small_below, Pr=2, Pc=2, pr=1, pc=0, beta0=1)
        assert got[1] == 8 * -(-mt * f // 8) * nt * f


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("pr,pc", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_rule_kept_tile_flops(hk, prec, pr, pc):
    """2 x 2 process grid, distribution blocks of 2 x 2 tiles (tpb_shift 1), 2 x 3 local blocks from row block 1."""
    grid = dict(rule=1, tpb_shift=1, rblk0=1, cblk0=0, pr=pr, Pr=2, pc=pc, Pc=2)
    got = agree(hk, prec, "RECT", 4, 6, 192, **grid)
    kept = 0
    for bi in range(2):
        for bj in range(3):
            gI, gJ = (1 + bi) * 2 + pr, bj * 2 + pc
            kept += 4 if gI > gJ else 3 if gI == gJ else 0
    assert got[3] == 2.0 * T * T * 192 * kept


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("small_below", [384, 1])
def test_range_and_trap_flops(hk, prec, small_below):
    sb = dict(small_below=small_below)
    for mt, nt in ((3, 2), (6, 4), (1, 6)):
        agree(hk, prec, "RECT", mt, nt, 2 * T, ktri=1, **sb)
        agree(hk, prec, "RECT", mt, nt, 8 * T, ktri=1, **sb)
    for mt, nt, krag0 in ((6, 3, 2), (5, 2, 0), (4, 6, 4), (4, 6, 9)):
        agree(hk, prec, "RECT", mt, nt, 6 * T, krag0=krag0, **sb)
    for mt, krag0 in ((4, 1), (6, 0), (6, 5)):
        agree(hk, prec, "LOWER", mt, mt, 6 * T, krag0=krag0, **sb)
    assert agree(hk, prec, "RECT", 6, 3, 6 * T, krag0=2, **sb)[3] == 2.0 * T * T * 3 * T * (6 * 6 - (1 + 2 + 3))
    for mt, nt in ((4, 4), (6, 6), (6, 4), (4, 6), (5, 6), (6, 2)):
        agree(hk, prec, "TRAP", mt, nt, 96 if prec == 64 else 128, **sb)
    assert agree(hk, prec, "TRAP", 6, 6, 128, **sb)[3] == 2.0 * T * T * 128 * (36 - 12)


@pytest.mark.parametrize("prec", [64, 32])
def test_tag(hk, prec):
    """mode * 1e8 + (K / 16) * 1e5 + min(128-tiles of one candidate, 99999), TRAP tagged as the RECT launch it is;
    K / 16 in both precisions."""
    assert agree(hk, prec, "RECT", 3, 5, 1056)[4] == 66 * 10 ** 5 + 15
    assert agree(hk, prec, "LOWER", 28, 28, 64)[4] == 10 ** 8 + 4 * 10 ** 5 + 406
    assert agree(hk, prec, "LAUUM", 5, 5, 640)[4] == 2 * 10 ** 8 + 40 * 10 ** 5 + 15
    assert agree(hk, prec, "TRAP", 4, 4, 128)[4] == 8 * 10 ** 5 + 16
    assert agree(hk, prec, "RECT", 1, 99999, 32)[4] == 2 * 10 ** 5 + 99999
    assert agree(hk, prec, "RECT", 400, 250, 32)[4] == 2 * 10 ** 5 + 99999  # 100000 tiles: clamped
    assert agree(hk, prec, "LOWER", 447, 447, 32)[4] == 10 ** 8 + 2 * 10 ** 5 + 99999  # 100128 tiles
    if prec == 64:
        assert agree(hk, 64, "RECT", 3, 5, 1056, k=8, bstride=1 << 24)[4] == 66 * 10 ** 5 + 15
