"""CPU side of tests/test_shard_kernels.py.
- The hooks of the kernels of the sharded path and of the rest of solve.hip refuse what a launch cannot honour, or the
  arrays do not cover, with GOGP_EARG BEFORE touching the device (device = -1 is enough to see it): every array one element
  short, a NULL array, and the shapes, grids and strides each launcher cannot take.
- The references of tests/shard_kernels_ref.py judge themselves on every shape the GPU test uses: the integer cases are
  exact in float64, and the float64 evaluation of the same operations passes the bounds the kernels are held to.
- The layout model: over each grid used, the ranks' tiles tile the global matrix exactly once.
- The manifest: every __global__ of solve.hip and dist2d.hip is mapped to the hook that tests it in isolation, or exempted
  by name with a reason; dist2d.hip launches its kernels through their launchers alone."""
import collections
import os
import re

import numpy as np
import pytest

import shard_kernels_ref as R
from gogp_amd import _lib
from test_substitution_kernels import judge, same_bits

EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
F64, F32, LD = np.float64, np.float32, np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP = dict(nb_shift=6, Pr=2, Pc=3, pr=1, pc=2)  # local tile 1 of grid row 1 of 2 is global tile 3: rows up to 255
T6 = 64 * 64

#: valid arguments of a small launch of every hook; an array's entry is its length, the SHORTEST the hook accepts
VALID = {
    "gather_rows": dict(MAP, rows=128, y=256, yloc=128),
    "gather_x": dict(MAP, D=3, n=100, rows=128, X=300, a=100, Xloc=384, aloc=128),
    "scatter_tile": dict(precision=64, nb=64, n=165, row0=128, col0=64, diag=0, r0=64, src=T6, dst=(165 - 64) * 165),
    "gather_rows_of_l": dict(MAP, precision=64, mloc=3, nloc=2, n=300, diag_only=0, Lch=6 * T6, rows=4, out=4 * 300),
    "scatter_stage": dict(precision=32, lds=136, nloc=2, mloc=3, bi=2, nb=64, stage=63 * 136 + 128, Lch=6 * T6),
    "transpose_rect": dict(precision=64, lds=104, ldd=40, rows=32, cols=96, src=31 * 104 + 96, dst=95 * 40 + 32),
    "transpose_sq": dict(precision=32, lds=72, ldd=64, n=64, src=63 * 72 + 64, dst=T6),
    "copy_block": dict(ld=72, nb=64, rows=5, dst=320, src=4 * 72 + 64),
    "residual_block": dict(precision=64, ld=72, nrecv=1, nb=64, rows=5, W=320, Ks=4 * 72 + 64, U=4 * 72 + 64, recv=320),
    "pack_blocks": dict(nblk=3, blk=10, first=1, stride=3, dst=30, src=80),
    "convert_block": dict(precision=64, precision2=32, lds=10, ldd=12, rows=3, cols=7, src=27, dst=31),
    "chunk_tdot": dict(precision=64, rows=300, nb=64, chunk=300 * 64, v=300, part=128, out=64),
    "chunk_alpha": dict(MAP, precision=64, mloc=3, nloc=2, Ych=6 * T6, z=384, out=384),
    "chunk_sumsq": dict(MAP, precision=64, mloc=3, nloc=2, n=300, Ych=6 * T6, part=192, out=1),
    "lml_scalars": dict(precision=64, ld=70, n=65, k=1, bstride=0, L=64 * 70 + 65, z=65, y=65, alpha=65, scalars=5),
    "alpha_from_y_batched": dict(ld=264, npad=256, k=2, bstride=70000, Y=70000 + 255 * 264 + 256, z=70256, alpha=70256),
    "trace_from_y": dict(ld=264, n=200, npad=256, Y=199 * 264 + 256, alpha=200, part=200, out=1),
    "zero_upper_blocks": dict(precision=64, ld=520, npad=512, k=1, bstride=0, R=511 * 520 + 512),
    "ydiag": dict(precision=64, ld=264, k=1, bstride=0, Dinv=65536, Y=255 * 264 + 256),
    "zero_block": dict(precision=64, ld=520, rows=3, cols=510, k=1, bstride=0, B=2 * 520 + 510),
    "extract_lower": dict(precision=64, ld=260, n=257, L=256 * 260 + 257, out=257 * 257),
    "pack_lower": dict(precision=64, n=257, npad=512, ld=520, src=257 * 257, L=511 * 520 + 512),
    "sigma": dict(m=5, prior=5, q=5, sigma=5),
    "logdet_block": dict(ld=72, row0=128, n=150, nb=64, L=63 * 72 + 64, acc=1),
    "dot": dict(n=300, a=300, b=300, out=1),
    "sumsq_info": dict(n=300, z=300, info=1, out=2),
    "vector_op": dict(op=1, precision=64, count=300, f=0.5, a=300, b=300),
}
ARRAY_KINDS = "aoAOPBfrn"
#: arrays that may be NULL (with length 0) in the valid call
MAY_BE_NULL = {("lml_scalars", "alpha"), ("sigma", "q"), ("sumsq_info", "info")}
#: arrays whose length is an argument of its own (the number of requested rows), not a minimum
ANY_LENGTH = {("gather_rows_of_l", "rows")}


@pytest.fixture(scope="module")
def hooks():
    _lib.build()
    return _lib.hooks()


def dtype_for(kind, a):
    if kind in "AOB":
        return F32 if a["precision"] == 32 else F64
    if kind == "P":
        return F32 if a["precision2"] == 32 else F64
    return {"f": F32, "r": np.int64}.get(kind, F64)


def call(hooks, which, **over):
    """The hook `which` on device -1 with VALID's arguments overridden by `over` (an array's entry: its length, or None for
    a NULL pointer); returns the status."""
    a = dict(VALID[which], **over)
    args, keep = [-1], []
    for name, kind in _lib.SHARD_HOOKS[which]:
        if kind in ARRAY_KINDS:
            arr = None if a[name] is None else np.zeros(max(a[name], 1), dtype_for(kind, a))
            keep.append(arr)
            ptr = None if arr is None else arr.ctypes.data
            if kind in "ao":
                ptr = None if arr is None else arr.ctypes.data_as(_lib._dp)
            args += [ptr, 0 if arr is None else a[name]]
        else:
            args.append(a[name])
    return getattr(hooks, "gogp_test_" + which)(*args)


def test_the_table_names_every_hook():
    assert set(VALID) == set(_lib.SHARD_HOOKS)
    for which, spec in _lib.SHARD_HOOKS.items():
        assert set(VALID[which]) == {name for name, _ in spec}, which


ARRAYS = [(w, name) for w, spec in _lib.SHARD_HOOKS.items() for name, kind in spec if kind in ARRAY_KINDS]


@pytest.mark.parametrize("which,name", ARRAYS, ids=["%s:%s" % a for a in ARRAYS])
def test_shard_hooks_refuse_short_and_null_arrays(hooks, which, name):
    short = call(hooks, which, **{name: VALID[which][name] - 1})
    assert short in OKS if (which, name) in ANY_LENGTH else short == EARG
    if (which, name) in MAY_BE_NULL:
        assert call(hooks, which, **{name: None}) in OKS
    else:
        assert call(hooks, which, **{name: None}) == EARG


BAD_MAP = [dict(pr=2), dict(pc=3), dict(pr=-1), dict(Pr=0), dict(Pc=9), dict(nb_shift=4), dict(nb_shift=11)]
BAD_TILES = [dict(mloc=4), dict(nloc=3), dict(mloc=0)]  # 4 x 2 local tiles on a 2 x 3 grid: 8 against 6 tiles
REFUSED = [(w, bad) for w in ("gather_rows", "gather_x", "gather_rows_of_l", "chunk_alpha", "chunk_sumsq") for bad in BAD_MAP]
# tile counts the grid does not divide: the product pads so that it does
REFUSED += [(w, bad) for w in ("gather_rows_of_l", "chunk_alpha", "chunk_sumsq") for bad in BAD_TILES]
REFUSED += [
    ("gather_rows", dict(rows=100)), ("gather_rows", dict(rows=0)),
    ("gather_x", dict(rows=100)), ("gather_x", dict(D=0)), ("gather_x", dict(D=65)), ("gather_x", dict(n=0)),
    ("scatter_tile", dict(precision=16)), ("scatter_tile", dict(row0=165)), ("scatter_tile", dict(col0=165)),
    ("scatter_tile", dict(r0=129)), ("scatter_tile", dict(r0=-1)), ("scatter_tile", dict(diag=2)), ("scatter_tile", dict(nb=0)),
    ("scatter_tile", dict(n=0)),
    ("gather_rows_of_l", dict(n=385)), ("gather_rows_of_l", dict(n=0)), ("gather_rows_of_l", dict(diag_only=2)),
    ("gather_rows_of_l", dict(diag_only=1)),  # the diagonal takes no rows
    ("scatter_stage", dict(bi=3)), ("scatter_stage", dict(bi=-1)), ("scatter_stage", dict(lds=127)),
    ("scatter_stage", dict(nb=0)), ("scatter_stage", dict(precision=8)),
    ("transpose_rect", dict(rows=33)), ("transpose_rect", dict(cols=95)), ("transpose_rect", dict(lds=95)),
    ("transpose_rect", dict(ldd=31)), ("transpose_rect", dict(rows=0)),
    ("transpose_sq", dict(n=48)), ("transpose_sq", dict(n=0)), ("transpose_sq", dict(lds=63)), ("transpose_sq", dict(ldd=63)),
    ("copy_block", dict(ld=63)), ("copy_block", dict(rows=0)), ("copy_block", dict(nb=0)),
    ("residual_block", dict(nrecv=-1)), ("residual_block", dict(ld=63)), ("residual_block", dict(rows=0)),
    ("residual_block", dict(nrecv=0)),  # no received blocks: recv must be NULL
    ("pack_blocks", dict(blk=9)),  # floats travel as doubles, pairs of doubles per load: an odd block loses its last one
    ("pack_blocks", dict(blk=0)), ("pack_blocks", dict(nblk=0)), ("pack_blocks", dict(first=-1)),
    ("pack_blocks", dict(stride=0)),
    ("convert_block", dict(precision=32)),  # float -> float has no instance
    ("convert_block", dict(precision=16)), ("convert_block", dict(rows=0)), ("convert_block", dict(cols=0)),
    ("convert_block", dict(lds=6)), ("convert_block", dict(ldd=6)),
    ("chunk_tdot", dict(nb=96)),  # the grid is nb / 64 column groups: columns 64 .. 95 would never be written
    ("chunk_tdot", dict(nb=32)), ("chunk_tdot", dict(nb=0)), ("chunk_tdot", dict(rows=0)),
    ("chunk_sumsq", dict(n=0)), ("chunk_sumsq", dict(n=385)),
    ("lml_scalars", dict(n=0)), ("lml_scalars", dict(ld=64)), ("lml_scalars", dict(k=0)), ("lml_scalars", dict(k=17)),
    ("lml_scalars", dict(k=2)),  # candidates need a stride
    ("lml_scalars", dict(k=2, bstride=4551, L=2 * 4551, z=4551 + 65, alpha=4551 + 65, scalars=4551 + 5)),  # odd
    ("lml_scalars", dict(precision=32, k=2, bstride=4552, L=2 * 4552, z=4552 + 65, alpha=4552 + 65, scalars=4552 + 5)),
    ("alpha_from_y_batched", dict(npad=255)), ("alpha_from_y_batched", dict(ld=263)), ("alpha_from_y_batched", dict(k=0)),
    ("alpha_from_y_batched", dict(bstride=0)), ("alpha_from_y_batched", dict(bstride=69999)),
    ("trace_from_y", dict(npad=255)), ("trace_from_y", dict(n=0)), ("trace_from_y", dict(n=257)),
    ("trace_from_y", dict(ld=255)),
    ("zero_upper_blocks", dict(npad=500)), ("zero_upper_blocks", dict(ld=519)), ("zero_upper_blocks", dict(ld=510)),
    ("zero_upper_blocks", dict(k=2)), ("zero_upper_blocks", dict(npad=0)),
    ("ydiag", dict(ld=255)), ("ydiag", dict(k=2)), ("ydiag", dict(precision=16)),
    ("zero_block", dict(cols=511)),  # pairs of columns are stored: an odd count writes one column more
    ("zero_block", dict(ld=519)), ("zero_block", dict(rows=0)), ("zero_block", dict(cols=0)), ("zero_block", dict(ld=508)),
    ("extract_lower", dict(n=0)), ("extract_lower", dict(ld=256)), ("extract_lower", dict(n=65536)),
    ("pack_lower", dict(n=0)), ("pack_lower", dict(n=513)), ("pack_lower", dict(ld=511)),
    ("sigma", dict(m=0)), ("logdet_block", dict(nb=0)), ("logdet_block", dict(ld=63)), ("logdet_block", dict(row0=-1)),
    ("dot", dict(n=0)), ("sumsq_info", dict(n=0)),
    ("vector_op", dict(op=7)), ("vector_op", dict(op=-1)), ("vector_op", dict(precision=32)),  # axpy has no float instance
    ("vector_op", dict(count=0)), ("vector_op", dict(op=6)),  # info_to_double converts one word
    ("vector_op", dict(op=0)), ("vector_op", dict(op=3)),  # fill and scale take no b
]


@pytest.mark.parametrize("which,bad", REFUSED, ids=["%s:%s" % (w, ",".join("%s=%s" % kv for kv in sorted(d.items())[:3]))
                                                    for w, d in REFUSED])
def test_shard_hooks_refuse(hooks, which, bad):
    assert call(hooks, which, **bad) == EARG


def test_shard_hooks_accept_the_valid_neighbours(hooks):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for which in VALID:
        assert call(hooks, which) in OKS, which
    big = dict(mloc=6, nloc=4, Ych=24 * T6)  # 6 x 4 local tiles on the 2 x 3 grid: 12 x 12 tiles
    for which, a in [("gather_rows", dict(pr=0, y=192)), ("gather_rows_of_l", dict(diag_only=1, rows=None, out=300)),
                     ("gather_rows_of_l", dict(n=384, out=4 * 384)), ("residual_block", dict(nrecv=0, recv=None)),
                     ("scatter_tile", dict(r0=128, dst=37 * 165)), ("scatter_stage", dict(bi=0)),
                     ("convert_block", dict(precision=32, precision2=64)), ("convert_block", dict(precision2=64)),
                     ("chunk_tdot", dict(nb=128, chunk=300 * 128, part=256, out=128)),
                     ("chunk_alpha", dict(big, z=768, out=768)), ("chunk_sumsq", dict(big, part=384)),
                     ("lml_scalars", dict(alpha=None)),
                     ("lml_scalars", dict(k=2, bstride=4552, L=4552 + 4545, z=4552 + 65, alpha=4552 + 65, scalars=4552 + 5)),
                     ("zero_upper_blocks", dict(npad=256, R=255 * 520 + 256)), ("zero_block", dict(cols=512, B=2 * 520 + 512)),
                     ("zero_block", dict(precision=32)), ("sumsq_info", dict(info=None, out=1)), ("sigma", dict(q=None)),
                     ("vector_op", dict(op=5, precision=32)), ("vector_op", dict(op=6, count=1)),
                     ("vector_op", dict(op=0, b=None)), ("vector_op", dict(op=3, b=None)),
                     ("trace_from_y", dict(n=256, Y=255 * 264 + 256, alpha=256, part=256))]:
        assert call(hooks, which, **a) in OKS, (which, a)


def test_scratch_of_chunk_tdot(hooks):
    from gogp_amd import gp
    for rows in R.TDOT_ROWS:
        for nb in R.TDOT_NB:
            assert gp.chunk_tdot_scratch(rows, nb) >= -(-rows // R.TDOT_SLAB) * nb
    for rows, nb in [(0, 64), (1, 96), (1, 0), (1, 2048)]:
        with pytest.raises(gp.GogpError):
            gp.chunk_tdot_scratch(rows, nb)


def test_wrapper_checks_names_and_types_before_the_hook(hooks):
    from gogp_amd import gp
    z = np.zeros
    with pytest.raises(TypeError):
        gp.shard_kernel_check("dot", a=z(4), b=z(4), n=4)  # out is missing
    with pytest.raises(TypeError):
        gp.shard_kernel_check("convert_block", precision=64, precision2=32, src=z(4, F32), lds=4, dst=z(4, F32), ldd=4,
                              rows=1, cols=4)  # src is not of `precision`
    with pytest.raises(gp.GogpError):
        gp.shard_kernel_check("dot", a=z(4), b=z(4), n=5, out=z(1))
    with pytest.raises(KeyError):
        gp.shard_kernel_check("nothing")


# ---- the layout model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pr,Pc", list(R.GRIDS))
@pytest.mark.parametrize("mult", [1, 2])
def test_the_ranks_tile_the_matrix_exactly_once(Pr, Pc, mult):
    NB, nb = R.num_tiles(Pr, Pc, mult), 4
    assert NB % Pr == 0 and NB % Pc == 0
    npad = NB * nb
    G = np.arange(npad * npad, dtype=F64).reshape(npad, npad)  # every element its own value
    seen = collections.Counter()
    rows_seen = collections.Counter()
    for pr in range(Pr):
        rows_seen.update(R.global_rows(NB, nb, Pr, pr).tolist())
        for pc in range(Pc):
            ch = R.chunks_of(G, nb, Pr, Pc, pr, pc, F64)
            assert ch.shape == (NB // Pc, NB // Pr, nb, nb)
            seen.update(ch.reshape(-1).tolist())
            # the chunk layout against the local matrix: chunk bj is the bj-th block column of the rank's tiles
            loc = R.local_matrix(G, nb, Pr, Pc, pr, pc)
            for bj in range(ch.shape[0]):
                assert np.array_equal(ch[bj].reshape(-1, nb), loc[:, bj * nb:(bj + 1) * nb])
    assert set(seen) == set(G.reshape(-1).tolist()) and set(seen.values()) == {1}, "a tile is lost or duplicated"
    assert set(rows_seen) == set(range(npad)) and set(rows_seen.values()) == {1}
    for pr, pc in R.GRIDS[(Pr, Pc)]:
        assert 0 <= pr < Pr and 0 <= pc < Pc
    # upper / lower select the tiles on and beyond the block diagonal
    for pr in range(Pr):
        for pc in range(Pc):
            ch = R.chunks_of(G, nb, Pr, Pc, pr, pc, F64, R.upper)
            vals = ch[~np.isnan(ch)]
            assert ((vals // npad) // nb <= (vals % npad) // nb).all()


# ---- the references judge themselves -------------------------------------------------------------------------------------------
def agree(got, want, e, exact, what):
    """The float64 evaluation against the reference: the same bits for the exact operands, within the bounds otherwise."""
    if isinstance(got, np.ndarray):
        got, want, e = (got,), (want,), (e,)
    for g, w, b in zip(got, want, e):
        g, w = np.asarray(g, F64).reshape(-1), np.asarray(w).reshape(-1)
        if exact:
            assert same_bits(g, w.astype(F64)), what
            assert np.array_equal(w, w.astype(F64).astype(LD)), what + ": the exact reference is no float64"
        elif np.abs(w).max() > 0:
            judge(g, w, np.asarray(b, F64).reshape(-1), what)  # (which also asserts the cap: max(e) <= 1e-10 max |want|)
        else:
            assert not g.any(), what


@pytest.mark.parametrize("case", R.SUMSQ_CASES, ids=lambda c: "nb%d-%dx%d-x%d" % (1 << c[0], c[1], c[2], c[3]))
def test_chunk_references(case):
    nb_shift, Pr, Pc, mult = case
    for exact in (True, False):
        p = R.layout_problem(nb_shift, Pr, Pc, mult, exact)
        nb, npad = p["nb"], p["npad"]
        for prec in (64, 32):
            G = R.rounded(p["G"], prec)
            if exact:
                assert np.array_equal(G, p["G"])
            for pr, pc in R.GRIDS[(Pr, Pc)]:
                rows, got, _, _ = R.chunk_alpha_eval(G, p["z"], nb, Pr, Pc, pr, pc, F64)
                rows2, want, e = R.chunk_alpha_ref(G, p["z"], nb, Pr, Pc, pr, pc)
                assert np.array_equal(rows, rows2)
                agree(got, want, e, exact, "chunk_alpha")
                for n in (R.sumsq_ns(nb, npad) if nb_shift == 6 else [npad - nb // 2 - 1]):
                    part, out, _ = R.chunk_sumsq_eval(G, nb, Pr, Pc, pr, pc, n, F64)
                    want, e = R.chunk_sumsq_ref(G, nb, Pr, Pc, pr, pc, n)
                    agree((part, np.array([out])), want, e, exact, "chunk_sumsq")
                    assert not part[R.global_rows(p["NB"], nb, Pr, pr) >= n].any()


def test_tdot_and_residual_references():
    for rows in R.TDOT_ROWS:
        for nb in R.TDOT_NB:
            for exact in (True, False):
                p = R.tdot_problem(rows, nb, exact)
                want, e = R.tdot_ref(p["C"], p["v"])
                agree(R.tdot_eval(p["C"], p["v"], F64), want, e, exact, "tdot rows%d nb%d" % (rows, nb))
    for nb in (64, 512):
        for rows in R.RESIDUAL_ROWS:
            for nrecv in R.RESIDUAL_NRECV:
                for exact in (True, False):
                    p = R.residual_problem(nb + 3 if rows is None else rows, nb, nrecv, exact)
                    want, e = R.residual_ref(p["Ks"], p["U"], p["recv"])
                    got = R.residual_eval(p["Ks"], p["U"], p["recv"], F64)
                    agree(got, want, e, exact, "residual")
                    if exact:  # the fp64 difference is exact, and does not fit a float: the float instance has to round
                        assert np.array_equal(p["Ks"], p["Ks"].astype(F32).astype(F64))
                        assert nrecv == 0 and rows == 1 or (got.astype(F32).astype(F64) != got).any()


def test_reduction_references():
    # (seeds 1 .. BATCH_K with the y of seed 1: the candidates of the batched launch, which share y)
    lml = [(n, 0, 0) for n in R.LML_N] + [(n, c + 1, 1) for n in R.LML_BATCHED_N for c in range(R.BATCH_K)]
    for n, seed, yseed in lml:
        for exact in (True, False):
            p = dict(R.lml_problem(n, exact, seed=seed), y=R.lml_problem(n, exact, seed=yseed)["y"])
            for a in (None, p["a"]):
                want, e = R.lml_ref(p["d"], p["z"], p["y"], a)
                got = R.lml_eval(p["d"], p["z"], p["y"], a, F64)
                judge(got[:1], want[:1], e[:1], "log-determinant")
                agree(got[1:3], want[1:3], e[1:3], exact, "z'z, y'alpha")
                assert same_bits(got[3:], want[3:].astype(F64))
    for n in R.TRACE_N:
        npad = R.up256(n)
        for exact in (True, False):
            p = R.rowblock_problem(n, npad, exact)
            Y = p["Y"].astype(F32).astype(F64)
            want, e = R.trace_ref(Y, p["a"])
            part, out, _ = R.trace_eval(Y, p["a"], F64)
            agree((part, np.array([out])), want, e, exact, "trace n%d" % n)
    for npad in (256, 512):
        for exact in (True, False):
            for c in range(R.BATCH_K):
                p = R.rowblock_problem(npad, npad, exact, seed=c + 1)
                want, e = R.alpha_ref(p["Y"], p["z"])
                agree(R.alpha_eval(p["Y"], p["z"], F64)[0], want, e, exact, "alpha_from_y")
    for n in R.REDUCE_N:
        for exact in (True, False):
            p = R.vec_problem(n, exact)
            for x, y in (("a", "b"), ("a", "a")):
                want, e = R.dot_ref(p[x], p[y])
                agree(R.dot_eval(p[x], p[y], F64), want, e, exact, "dot n%d" % n)
    d = np.random.default_rng(31).uniform(1.5, 4.0, 512)
    for live in (0, 1, 35, 259, 512):
        want, e = R.logdet_ref(d, live, 3.25)
        judge(R.logdet_eval(d, live, 3.25, F64), want, e, "logdet")
    for m in R.SIGMA_M:
        for exact in (True, False):
            p = R.sigma_problem(m, exact)
            assert (p["prior"] > p["q"]).all() or exact and (p["prior"] >= p["q"]).all()
            want, e = R.sigma_ref(p["prior"], p["q"])
            agree(R.sigma_eval(p["prior"], p["q"], F64), want, e, exact, "sigma")


# ---- the manifest ----------------------------------------------------------------------------------------------------------------
#: kernel -> the hook (gogp_test_<name>) that drives it through its product launcher
KERNEL_HOOKS = {
    # solve.hip
    "trsv_fwd_kernel": "trsv_steps", "trsv_bwd_kernel": "trsv_steps", "alpha_from_y_kernel": "alpha_from_y",
    "lml_scalars_kernel": "lml_scalars", "rownorm_dot_kernel": "rownorm_dot", "trace_rows_kernel": "trace_from_y",
    "sum_kernel": "trace_from_y",  # no launcher of its own: n = 1023 .. 2049 of trace_from_y, and chunk_sumsq on 1088 rows
    "zero_upper_kernel": "zero_upper_blocks", "ydiag_kernel": "ydiag", "tinv_init_kernel": "tinv",
    "blockmm_kernel": "blockmm", "zero_block_kernel": "zero_block", "fill_kernel": "vector_op", "axpy_kernel": "vector_op",
    "dot_kernel": "dot", "extract_lower_kernel": "extract_lower", "convert_block_kernel": "convert_block",
    "pack_lower_kernel": "pack_lower", "sigma_kernel": "sigma", "transpose_sq_kernel": "transpose_sq",
    "pack_blocks_kernel": "pack_blocks", "chunk_tdot_kernel": "chunk_tdot", "chunk_tdot_finish_kernel": "chunk_tdot",
    "chunk_alpha_kernel": "chunk_alpha", "chunk_rowsq_kernel": "chunk_sumsq", "logdet_block_kernel": "logdet_block",
    "sumsq_info_kernel": "sumsq_info", "info_to_double_kernel": "vector_op",
    # dist2d.hip
    "residual_from_kernel": "vector_op", "gather_rows_kernel": "gather_rows", "scatter_tile_kernel": "scatter_tile",
    "gather_rows_of_l_kernel": "gather_rows_of_l", "scatter_stage_kernel": "scatter_stage", "gather_x_kernel": "gather_x",
    "transpose_rect_kernel": "transpose_rect", "add_inplace_kernel": "vector_op", "scale_kernel": "vector_op",
    "copy_block_kernel": "copy_block", "residual_block_kernel": "residual_block", "add_vec_kernel": "vector_op",
}
#: kernels without a hook, each with its reason
EXEMPT = {"selftest_fill_kernel": "the payload of gogp_dist_selftest, which checks every element it delivers on the host"}
#: the tests that drive each hook: a kernel counts as tested in isolation only if its hook is called there
HOOK_TESTS = ("test_shard_kernels.py", "test_substitution_kernels.py")


def kernels_of(name):
    src = open(os.path.join(ROOT, "gogp_amd", "csrc", name)).read()
    src = re.sub(r"//[^\n]*", "", src)
    return src, re.findall(r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\(", src)


def test_every_kernel_of_the_two_files_is_tested_in_isolation_or_exempt():
    found = kernels_of("solve.hip")[1] + kernels_of("dist2d.hip")[1]
    assert len(found) == len(set(found)) >= 40
    assert found.count("selftest_fill_kernel") == 1
    missing = [k for k in found if k not in KERNEL_HOOKS and k not in EXEMPT]
    assert not missing, "kernels without a hook: add one (include/gogp_testhooks.h) and name it here: %s" % missing
    assert not set(KERNEL_HOOKS) & set(EXEMPT)
    assert set(KERNEL_HOOKS) | set(EXEMPT) == set(found), "the table names kernels that are gone"
    assert set(EXEMPT) == {"selftest_fill_kernel"} and all(EXEMPT.values())
    declared = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    tests = "".join(open(os.path.join(ROOT, "tests", t)).read() for t in HOOK_TESTS)
    for kernel, hook in KERNEL_HOOKS.items():
        assert "gogp_test_" + hook in declared, (kernel, hook)
        used = '"%s"' % hook if hook in _lib.SHARD_HOOKS else hook + "_check("
        assert used in tests, "no test calls the hook of %s" % kernel
    # every op of the shared vector hook is exercised by name
    shard = open(os.path.join(ROOT, "tests", "test_shard_kernels.py")).read()
    for op in _lib.VECTOR_OPS:
        assert re.search(r'\b%s\b' % op, shard), op
    # a kernel added later is found: the scan sees a templated and a plain one
    probe = "template <class T>\n__global__ __launch_bounds__(256) void new_kernel(T *p) {}\n__global__ void other_kernel() {}"
    assert re.findall(r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\(", probe) == ["new_kernel",
                                                                                                          "other_kernel"]


def test_dist2d_launches_its_kernels_through_their_launchers():
    src, kernels = kernels_of("dist2d.hip")
    for k in kernels:
        if k in EXEMPT:
            continue
        sites = len(re.findall(r"hipLaunchKernelGGL\(\s*\(?%s\b" % k, src))
        assert sites == (2 if k == "add_inplace_kernel" else 1), "%s is launched at %d places" % (k, sites)
    # ... and each launch site sits in a launcher (launch_* or the template behind its overloads)
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?(\w+)", src):
        if m.group(1) in EXEMPT:
            continue
        head = re.findall(r"\n(?:static )?void (?:gogp::)?(\w+)\(", src[:m.start()])[-1]
        assert head.startswith("launch_") or head.endswith("_t"), (m.group(1), head)
    hdr = open(os.path.join(ROOT, "gogp_amd", "csrc", "common.h")).read()
    for k in kernels:
        if k not in EXEMPT:
            assert re.search(r"\bvoid launch_%s\(" % k[:-len("_kernel")], hdr), k
