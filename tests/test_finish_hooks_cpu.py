"""CPU side of tests/test_finish_kernels.py.
- The hooks of the leave-one-out, multi-output and sparse finishing kernels refuse what a launch cannot honour, or the arrays
  do not cover, with GOGP_EARG BEFORE touching the device (device = -1 is enough to see it): every array one element short,
  a NULL array, and the shapes and strides each launcher cannot take.
- The references of tests/finish_kernels_ref.py judge themselves on every shape the GPU test uses: the integer cases are exact
  in float64 (the float64 evaluation has the bits of the long-double one), and the float64 evaluation of the same operations
  passes the bounds the kernels are held to, with every bound under the cap of judge().
- A replica of the (slot, row) stores of loo_scale_symv_kernel covers every pair of upart exactly once."""
import collections

import numpy as np
import pytest

import finish_kernels_ref as R
from gogp_amd import _lib
from test_substitution_kernels import judge, same_bits

EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)
F64, LD = np.float64, np.longdouble
SQ = 256 * 256
MMAX = 4 * 65535

#: valid arguments of a small launch of every hook; an array's entry is its length, the SHORTEST the hook accepts
VALID = {
    "loo_stats": dict(ld=264, n=200, npad=256, Kinv=255 * 264 + 256, alpha=200, y=200, mu=200, sigma=200, logp=200, v=256,
                      sc=256, part=1),
    "loo_scale_symv": dict(ld=264, n=200, npad=256, ldb=272, Kinv=255 * 264 + 256, sc=256, v=256, B=255 * 272 + 256,
                           upart=4 * 256, u=256),
    "loo_rank2": dict(ld=264, n=200, npad=256, G=255 * 264 + 256, u=256, alpha=200),
    "multi_dots": dict(ld=256, n=200, T=3, Yt=2 * 256 + 200, At=2 * 256 + 200, dots=3),
    "sparse_finish_b": dict(Mp=256, inv_s2=0.5, Bacc=SQ, B=SQ),
    "sparse_copy_upper": dict(Mp=256, src=SQ, dst=SQ),
    "sparse_weights": dict(Mp=256, s4=0.5, B=SQ, Binv=SQ, g=256, T=SQ, S=SQ),
    "sparse_multi_weights": dict(Mp=256, T=3, s4=0.5, B=SQ, Binv=SQ, GG=SQ, Tm=SQ, S=SQ),
    "sparse_scalars": dict(M=100, Mp=128, C=99 * 128 + 100, B=99 * 128 + 100, Binv=99 * 128 + 100, r=100, g=100, out=5),
    "sparse_sumsq": dict(n=300, y=300, out=1),
    "sparse_predict": dict(ld=70, ncols=65, m=5, A=4 * 70 + 65, V=4 * 70 + 65, prior=5, q=5, dot=5, inv_s2=0.5, mu=5, sigma=5),
    "sparse_multi_sigma": dict(ld=70, ncols=65, m=5, A=4 * 70 + 65, V=4 * 70 + 65, prior=5, q=5, sigma=5),
    "sparse_multi_dots": dict(ld=300, M=257, T=5, tstride=7, Rt=4 * 300 + 257, Gt=4 * 300 + 257, out=12),
    "sparse_multi_sumsq": dict(ldy=8, n=300, T=5, Y=299 * 8 + 5, out=5),
    "sparse_multi_pad": dict(ldy=8, rows=100, T=5, kp=16, rpad=128, ldp=24, Y=99 * 8 + 5, Yp=127 * 24 + 16),
}
ELEMENTWISE = ("sparse_finish_b", "sparse_copy_upper", "sparse_weights", "sparse_multi_weights")


@pytest.fixture(scope="module")
def hooks():
    _lib.build()
    return _lib.hooks()


def call(hooks, which, **over):
    """The hook `which` on device -1 with VALID's arguments overridden by `over` (an array's entry: its length, or None for
    a NULL pointer); returns the status."""
    a = dict(VALID[which], **over)
    args, keep = [-1], []
    for name, kind in _lib.FINISH_HOOKS[which]:
        if kind in "ao":
            arr = None if a[name] is None else np.zeros(max(a[name], 1))
            keep.append(arr)
            args += [None if arr is None else arr.ctypes.data_as(_lib._dp), 0 if arr is None else a[name]]
        else:
            args.append(a[name])
    return getattr(hooks, "gogp_test_" + which)(*args)


def test_the_table_names_every_hook():
    assert set(VALID) == set(_lib.FINISH_HOOKS)
    for which, spec in _lib.FINISH_HOOKS.items():
        assert set(VALID[which]) == {name for name, _ in spec}, which


ARRAYS = [(w, name) for w, spec in _lib.FINISH_HOOKS.items() for name, kind in spec if kind in "ao"]


@pytest.mark.parametrize("which,name", ARRAYS, ids=["%s:%s" % a for a in ARRAYS])
def test_finish_hooks_refuse_short_and_null_arrays(hooks, which, name):
    assert call(hooks, which, **{name: VALID[which][name] - 1}) == EARG
    assert call(hooks, which, **{name: None}) == EARG


LOO = ("loo_stats", "loo_scale_symv", "loo_rank2")
REFUSED = [(w, bad) for w in LOO for bad in (dict(n=257), dict(n=0), dict(npad=255, n=100), dict(npad=0), dict(npad=320),
                                             dict(ld=255), dict(npad=65536))]
REFUSED += [("loo_scale_symv", dict(ldb=255)),
            ("multi_dots", dict(T=0)), ("multi_dots", dict(T=129)), ("multi_dots", dict(n=0)), ("multi_dots", dict(ld=199))]
# the four Mp x Mp launchers start Mp / 256 workgroups per row: any other Mp would drop columns without a word
REFUSED += [(w, bad) for w in ELEMENTWISE for bad in (dict(Mp=255), dict(Mp=192), dict(Mp=64), dict(Mp=0), dict(Mp=4096 + 256))]
REFUSED += [("sparse_finish_b", dict(inv_s2=np.inf)), ("sparse_weights", dict(s4=np.nan)),
            ("sparse_multi_weights", dict(T=0)), ("sparse_multi_weights", dict(T=129)),
            ("sparse_scalars", dict(M=0)), ("sparse_scalars", dict(M=129)), ("sparse_scalars", dict(Mp=99)),
            ("sparse_scalars", dict(Mp=4097, M=100)),
            ("sparse_sumsq", dict(n=0)),
            ("sparse_multi_dots", dict(tstride=4)),           # tstride < T
            ("sparse_multi_dots", dict(ld=256)),              # ld < M
            ("sparse_multi_dots", dict(M=0)), ("sparse_multi_dots", dict(T=0)), ("sparse_multi_dots", dict(M=4097)),
            ("sparse_multi_sumsq", dict(ldy=4)),              # ldy < T
            ("sparse_multi_sumsq", dict(n=0)), ("sparse_multi_sumsq", dict(T=129)),
            ("sparse_multi_pad", dict(rpad=120)),             # rpad * kp = 1920: the launcher would return without a launch
            ("sparse_multi_pad", dict(kp=17, ldp=24, Yp=127 * 24 + 17)),
            ("sparse_multi_pad", dict(ldp=15)),               # ldp < kp
            ("sparse_multi_pad", dict(ldy=4)),                # ldy < T
            ("sparse_multi_pad", dict(rows=129)), ("sparse_multi_pad", dict(rows=0)), ("sparse_multi_pad", dict(T=17)),
            ("sparse_multi_pad", dict(T=0))]
BIG = dict(ld=1, ncols=1, m=MMAX + 1, A=MMAX + 1, V=MMAX + 1, prior=MMAX + 1, q=MMAX + 1)
REFUSED += [("sparse_predict", dict(BIG, dot=MMAX + 1, mu=MMAX + 1, sigma=MMAX + 1)),  # one wave per point, 4 per workgroup
            ("sparse_multi_sigma", dict(BIG, sigma=MMAX + 1)),
            ("sparse_predict", dict(m=0)), ("sparse_predict", dict(ncols=0)), ("sparse_predict", dict(ld=64)),
            ("sparse_predict", dict(inv_s2=np.inf)),
            ("sparse_multi_sigma", dict(m=0)), ("sparse_multi_sigma", dict(ld=64))]


@pytest.mark.parametrize("which,bad", REFUSED, ids=["%s:%s" % (w, ",".join("%s=%s" % kv for kv in sorted(d.items())[:3]))
                                                    for w, d in REFUSED])
def test_finish_hooks_refuse(hooks, which, bad):
    assert call(hooks, which, **bad) == EARG


def test_finish_hooks_accept_the_valid_neighbours(hooks):
    # the same calls with the offending argument fixed are not refused (no GPU here: GOGP_EHIP, on a GPU: GOGP_OK)
    for which in VALID:
        assert call(hooks, which) in OKS, which
    ok = dict(BIG, m=MMAX)
    for which, a in [("loo_stats", dict(n=256, alpha=256, y=256, mu=256, sigma=256, logp=256)), ("loo_stats", dict(n=1)),
                     ("loo_scale_symv", dict(n=256)), ("loo_scale_symv", dict(ld=256, ldb=256)), ("loo_rank2", dict(n=1)),
                     ("multi_dots", dict(T=1)), ("multi_dots", dict(n=1, ld=1)),
                     ("sparse_scalars", dict(M=128, C=SQ, B=SQ, Binv=SQ, r=128, g=128)),
                     ("sparse_multi_dots", dict(tstride=5, out=10)), ("sparse_multi_sumsq", dict(ldy=5, Y=300 * 5)),
                     ("sparse_multi_pad", dict(rows=128, Y=128 * 8)), ("sparse_multi_pad", dict(T=16, ldy=16, Y=100 * 16)),
                     ("sparse_multi_pad", dict(ldp=16, Yp=128 * 16)),
                     ("sparse_predict", dict(ok, dot=MMAX, mu=MMAX, sigma=MMAX)), ("sparse_multi_sigma", dict(ok, sigma=MMAX))]:
        assert call(hooks, which, **a) in OKS, (which, a)


def test_wrapper_checks_names_and_types_before_the_hook(hooks):
    from gogp_amd import gp
    z = np.zeros
    with pytest.raises(TypeError):
        gp.finish_check("sparse_sumsq", y=z(4), n=4)  # out is missing
    with pytest.raises(TypeError):
        gp.finish_check("sparse_sumsq", y=z(4, np.float32), n=4, out=z(1))
    with pytest.raises(gp.GogpError):
        gp.finish_check("sparse_sumsq", y=z(4), n=5, out=z(1))
    with pytest.raises(KeyError):
        gp.finish_check("sparse_nothing")


# ---- the (slot, row) stores of loo_scale_symv_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [4, 8, 20])
def test_every_slot_row_of_upart_is_written_once(nt):
    seen = collections.Counter(R.symv_slots(nt))
    assert set(seen) == {(s, r) for s in range(nt) for r in range(64 * nt)} and set(seen.values()) == {1}
    # the wrong slot the issue names -- the column sums to slot tj -- collides with the diagonal tile's and leaves holes
    wrong = collections.Counter(R.symv_slots(nt, column_slot_tj=True))
    assert max(wrong.values()) > 1 and len(wrong) < nt * nt * 64


# ---- the references judge themselves -----------------------------------------------------------------------------------------
def agree(eval_, ref, exact, what):
    """The float64 evaluation against the reference: the same bits for the exact operands, within the bounds otherwise."""
    got = eval_(F64)
    want, e = ref()
    if isinstance(got, np.ndarray):
        got, want, e = (got,), (want,), (e,)
    for g, w, b in zip(got, want, e):
        if exact:
            assert same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w.astype(F64))), what
            assert np.array_equal(w, w.astype(F64).astype(LD)), what + ": the exact reference is no float64"
        else:
            judge(g, w, b, what)  # (which also asserts the cap: max(e) <= 1e-10 max |want|)


@pytest.mark.parametrize("npad,n", R.STATS_CASES)
def test_stats_reference(npad, n):
    for exact in (True, False):
        p = R.stats_problem(npad, n, exact)
        got = R.stats_eval(p["kap"], p["a"], p["y"], npad, F64)
        want, e = R.stats_ref(p["kap"], p["a"], p["y"], npad)
        for g, w, b, name in zip(got, want, e, ("mu", "sigma", "logp", "v", "sc", "part")):
            judge(g, w, None if exact and name in ("mu", "sigma", "v") else b, name)
        assert not got[3][n:].any() and not got[4][n:].any()


@pytest.mark.parametrize("npad,n", R.SYMV_CASES + R.RANK2_CASES + [R.SYMV_EXACT_ONLY])
def test_loo_matrix_references(npad, n):
    for exact in (True, False):
        if (npad, n) in R.SYMV_CASES or exact:
            p = R.symv_problem(npad, n, exact)
            agree(lambda dt: R.symv_eval(p["K"], p["sc"], p["v"], npad, dt), lambda: R.symv_ref(p["K"], p["sc"], p["v"], npad),
                  exact, "symv")
        if (npad, n) in R.RANK2_CASES:
            q = R.rank2_problem(npad, n, exact)
            agree(lambda dt: R.rank2_eval(q["G"], q["u"], q["alpha"], dt), lambda: R.rank2_ref(q["G"], q["u"], q["alpha"]),
                  exact, "rank2")


def test_dot_references():
    shapes = [(1, T, n) for n, T in R.DOTS_CASES] + [(2, 1, n) for n in R.SUMSQ_N]
    shapes += [(3, T, n) for n in R.SUMSQ_N for T in R.SUMSQ_T] + [(4, T, M) for M, T in R.MDOTS_CASES]
    for tag, rows, k in shapes:
        for exact in (True, False):
            p = R.dots_problem(tag, rows, k, exact)
            pairs = {1: [("A", "B")], 2: [("A", "A")], 3: [("A", "A")], 4: [("A", "B"), ("B", "B")]}[tag]
            for x, y in pairs:
                agree(lambda dt: R.dots_eval(p[x], p[y], dt), lambda: R.dots_ref(p[x], p[y]), exact,
                      "dots %s" % ((tag, rows, k),))


@pytest.mark.parametrize("Mp", R.MPS)
def test_square_references(Mp):
    for exact in (True, False):
        s4 = R.S4_DYADIC if exact else R.S4_PLAIN
        p = R.square_problem(1, Mp, exact)
        agree(lambda dt: R.finish_b_eval(p["B"], s4, dt), lambda: R.finish_b_ref(p["B"], s4), exact, "finish_b")
        p = R.square_problem(3, Mp, exact)
        agree(lambda dt: R.weights_eval(p["B"], p["Binv"], p["g"], s4, dt),
              lambda: R.weights_ref(p["B"], p["Binv"], p["g"], s4), exact, "weights")
        p = R.square_problem(4, Mp, exact)
        for nT in R.NTS:
            agree(lambda dt: R.multi_weights_eval(p["B"], p["Binv"], p["GG"], nT, s4, dt),
                  lambda: R.multi_weights_ref(p["B"], p["Binv"], p["GG"], nT, s4), exact, "multi_weights T%d" % nT)


def test_scalars_and_predict_references():
    for M in R.SCALARS_M:
        for exact in (True, False):
            p = R.scalars_problem(M, exact)
            got = R.scalars_eval(p["c"], p["b"], p["bi"], p["r"], p["g"], F64)
            want, e = R.scalars_ref(p["c"], p["b"], p["bi"], p["r"], p["g"])
            judge(got[:1], want[:1], e[:1], "sum 2 log C_ii")
            judge(got[1:], want[1:], None if exact else e[1:], "out[1 .. 4]")
            assert (e <= 1e-10 * np.abs(want).astype(F64)).all()
    for m, ncols in R.PREDICT_CASES:
        for exact in (True, False):
            p = R.predict_problem(m, ncols, exact)
            a = (p["A"], p["V"], p["prior"], p["q"], p["dot"], p["inv_s2"])
            agree(lambda dt: R.predict_eval(*a, dt), lambda: R.predict_ref(*a), exact, "predict m%d ncols%d" % (m, ncols))
