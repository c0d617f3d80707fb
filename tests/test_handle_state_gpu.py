"""ONE handle across call families: no stored result goes stale, no reader changes what a later call returns, no writer
leaves behind what belonged to what it replaced.  Vocabulary, state model and twin: tests/handle_state_ref.py.

  reader after reader   6 origins x n = 300, 100 x 29 readers A: one handle per (origin, n, A), on it A B1 A B2 ... over every
                        reader B; every result equals the twin's (origin, then that call alone on a fresh handle), and its
                        kind -- value, GOGP_ESTATE, GOGP_EARG -- is what handle_state_ref.EXPECT says.  Five
                        origins carry noise variances where the library takes them (LaplaceObserve refuses them); the
                        sixth, ObservePlain, is Observe without, so that the candidates path runs on a regression state.
  writer after reader   origins Observe and Laplace at n = 300, every writer W: per reader A a handle with origin, A, W, then
                        every reader once, each equal to the twin's (origin, W, that reader) and of the kind the state
                        model gives; W's own results (an LML, a bound) equal the twin's too.
  the two suspects      test_laplace_fit_survives_a_candidates_call, test_gradient_after_candidates_behind_an_eager_observe
  failure paths         an Append that is not positive definite and a LaplaceObserve that does not converge, after readers
                        of every family have run.
  references            every reader's result on the fresh twin against the numpy reference of its family, so that "equal
                        to a fresh handle" means "right".

The comparison is bitwise throughout.  Determinism is measured, not assumed: the fixture `repeatable` runs every call of
the vocabulary, readers and writers, on two fresh handles in the same state and fails unless the labels whose bits differ
are exactly those listed in TOLERANT (none at present: every call returned the same bits twice on the MI355X).

The Basis* calls form K^-1 H "from the explicit K^-1 where a gradient has left it on the device (the default), or always
from the factor" (GP.SetBasis, option "basis_symm"), and take that route at their first call behind a factorisation: by
default a reader that forms K^-1 (Gradient, LOO, BlockCV, NoiseVariancesGradient, MultiGradient) moves later Basis
results by rounding (1e-13 measured), by design.  So the route is part of the state: where the origin's factor is Observe's,
K^-1 is there from the start and the handles keep the default; on every other origin and in the writer-after-reader cases
the handle and its twin pin the route (basis_symm_of), both values in turn over the cases.  Every test prints the
largest difference per compared label."""
import numpy as np
import pytest

import basis_ref as BR
import blockcv_ref as BC
import cg_lml_ref as CL
import grad_reduce_ref as GR
import handle_state_ref as S
import laplace_ref as LP
import loo_ref as LR
import multi_output_ref as MO
import noise_variances_ref as NV
import produce_grad_ref as PG
import select_inducing_ref as SI
import sparse_multi_ref as SM
import sparse_ref as SR
from gogp_amd import _lib, kernel
from gogp_amd import vecchia as VT

pytestmark = pytest.mark.gpu

#: label -> the measured fresh-against-fresh difference of a call that does not repeat its bits; such a label is compared
#: at rtol = 1e-6, atol = 1e-8 (a gradient: 1e-6 of its largest component)
TOLERANT = {}
#: labels that today's tests already compare bitwise across handles: they may not be listed above
BITWISE = {"LML", "Alpha", "L", "Produce", "ProduceCovariance", "Sample", "Gradient", "SparseObserve", "SparseGradient",
           "MultiLML", "CGAlpha", "CGProduce", "VecchiaGradient", "VecchiaProduceNearest"}
assert not BITWISE & set(TOLERANT)
KINV_FROM_THE_START = ("Observe", "ObservePlain")


def basis_symm_of(origin, n):
    """The option "basis_symm" of a reader-after-reader case: the default where K^-1 exists from the start, else pinned --
    1 (from K^-1) at n = 300, 0 (from the factor) at n = 100."""
    return None if origin in KINV_FROM_THE_START else (1 if n == 300 else 0)


#: ... and of the writer-after-reader cases, where a writer may drop K^-1: pinned on both origins, one value each
WRITER_BASIS_SYMM = {"Observe": 0, "Laplace": 1}

_TWINS = {}


def twin(n, seq, call, free=0, basis_symm=None):
    """The call's result on a fresh handle after the writers of seq, of which the last `free` may be refused: computed
    once per (n, writers, option, call), read only."""
    plan = S.twin_plan(seq, free)
    key = (n, tuple(plan), basis_symm, call)
    if key not in _TWINS:
        h = S.replay(n, plan, basis_symm)
        _TWINS[key] = S.apply(h, call)
        h.close()
    return _TWINS[key]


def check(got, want, expected, tag, worst):
    diffs = S.compare(got, want, tuple(TOLERANT), tag)
    for label, d in diffs.items():
        worst[label] = max(worst.get(label, 0.0), d)
    if expected is not None:
        for (label, out), (_, tw) in zip(got, want):
            says = expected(label) if callable(expected) else expected
            assert S.kind_of(out) == says == S.kind_of(tw), "%s %s: %s, the documents say %s" % (tag, label, S.kind_of(out), says)


def report(tag, worst, compared):
    print("%s: %d results compared; largest |handle - twin| per label: %s"
          % (tag, compared, ", ".join("%s %.3e" % kv for kv in sorted(worst.items())) or "(refusals only)"))


@pytest.fixture(scope="module")
def repeatable():
    """Every call of the vocabulary on two fresh handles in the same state, in the three states in which every reader
    returns values somewhere: the readers and the writers of the cases behind the origin, and the origin's own writers
    (two replays' logs).  Returns the labels whose bits differ, with the difference."""
    found = {}

    def measure(tag, first, second):
        for (label, a), (_, b) in zip(first, second):
            assert S.kind_of(a) == S.kind_of(b), (tag, label)
            if a[0] == "value" and not all(S.same_bits(u, v) for u, v in zip(a[1], b[1])):
                found[label] = max(found.get(label, 0.0), S.largest_difference(a[1], b[1]))

    for origin, n in (("ObservePlain", 300), ("Laplace", 300), ("Observe", 100)):
        seq = S.origin_sequence(origin, n)
        logs = []
        for _ in range(2):
            h = S.replay(n, seq)
            logs.append(h.log)
            h.close()
        for (name, first), (_, second) in zip(*logs):
            measure((origin, n, name), first, second)
        for call in S.READER_NAMES + S.WRITER_NAMES:
            h = S.replay(n, seq)
            again = S.apply(h, call)
            h.close()
            measure((origin, n, call), again, twin(n, seq, call))
    print("fresh against fresh: %s" % (found or "every label repeats its bits"))
    assert set(found) == set(TOLERANT), (found, TOLERANT)
    return found


# ---- reader after reader ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,n,a", S.pair_cases(), ids=["%s-%d-%s" % c for c in S.pair_cases()])
def test_reader_after_reader(origin, n, a, repeatable):
    seq, symm = S.origin_sequence(origin, n), basis_symm_of(origin, n)
    h = S.replay(n, seq, symm)
    worst, compared = {}, 0
    try:
        for b in S.READER_NAMES:
            for call in (a, b):  # (A again before each B: the chain A B1 A B2 ... also holds every B -> A)
                check(S.apply(h, call), twin(n, seq, call, basis_symm=symm), S.EXPECT[(origin, n, call)],
                      "%s n = %d, %s then %s: %s" % (origin, n, a, b, call), worst)
                compared += 1
    finally:
        h.close()
    report("%s n = %d A = %s" % (origin, n, a), worst, compared)


# ---- writer after reader ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,w", S.writer_cases(), ids=["%s-%s" % c for c in S.writer_cases()])
def test_writer_after_reader(origin, w, repeatable):
    n, symm = 300, WRITER_BASIS_SYMM[origin]
    seq = S.origin_sequence(origin, n)
    model = S.model_after(seq + [w])
    worst, compared = {}, 0
    for a in S.READER_NAMES:
        h = S.replay(n, seq, symm)
        try:
            S.apply(h, a)
            tag = "%s, %s, %s" % (origin, a, w)
            check(S.apply(h, w), twin(n, seq, w, basis_symm=symm), None, tag, worst)
            for b in S.READER_NAMES:
                check(S.apply(h, b), twin(n, seq + [w], b, free=1, basis_symm=symm), lambda label, b=b: S.expect(model, b, label),
                      "%s: %s" % (tag, b), worst)
                compared += 1
        finally:
            h.close()
    report("%s W = %s" % (origin, w), worst, compared)


# ---- the two suspects ------------------------------------------------------------------------------------------------------
LAPLACE_READERS = ("LaplaceGradient", "LaplaceMode", "LaplaceProduce")


@pytest.mark.parametrize("gradient_first", [False, True], ids=["fit", "fit_and_gradient"])
def test_laplace_fit_survives_a_candidates_call(gradient_first):
    """LaplaceObserve, observe_gradient_candidates (twice: the second replays the graph), then the Laplace readers: the
    fit's own bits.  The candidates work in their arena and leave "the GP's own state" alone; with gradient_first the
    gradient's weight matrix is already in bufA and its value cached."""
    n, seq = 300, ["LaplacePoisson"]
    h = S.replay(n, seq)
    worst = {}
    if gradient_first:
        check(S.apply(h, "LaplaceGradient"), twin(n, seq, "LaplaceGradient"), "value", "before", worst)
    cand = S.apply(h, "Candidates")
    check(cand, twin(n, seq, "Candidates"), "value", "the candidates on the counts", {})
    for r in LAPLACE_READERS:
        check(S.apply(h, r), twin(n, seq, r), "value", "after the candidates: %s" % r, worst)
    h.close()
    report("Laplace fit after candidates", worst, len(LAPLACE_READERS))


@pytest.mark.parametrize("n,options", [(300, {}), (300, {"kinv_split": 0}), (600, {"kinv_fused": 0}),
                                       (600, {"kinv_fused": 0, "kinv_split": 0})],
                         ids=["default", "kinv_split0", "unfused600", "unfused600_kinv_split0"])
def test_gradient_after_candidates_behind_an_eager_observe(n, options):
    """Observe (eager: K^-1 still accumulating behind the sweep), the candidates, then Gradient and the calls that read
    K^-1: the bits of Observe + that call on a fresh handle.  With "kinv_fused" = 0 at n = 600 (npad = 768) the sweep
    launches the first 512 columns' part of K^-1 by option "kinv_split" and Gradient would add the rest: the case of a
    partly accumulated bufA, which n = 300 (K^-1 fused into the sweep below npad = 10240) does not reach."""
    X, y, *_ = S.WR.inputs()

    def start():
        h = S.Handle(300)
        for k, v in options.items():
            h.g.set_option(k, v)
        h.g.X, h.g.Y = X[:n], y[:n]
        lml = h.g.Observe(h.x("observe1"))
        return h, lml

    readers = ("Gradient", "LOO", "LOOGradient", "NoiseVariancesGradient", "Produce5", "LML")
    want = {}
    for r in readers:
        t, lml_t = start()
        want[r] = S.apply(t, r)
        t.close()
    for first in readers[:3]:
        h, lml = start()
        assert lml == lml_t
        cand = S.apply(h, "Candidates")
        assert all(S.kind_of(o) == "value" for _, o in cand)
        worst = {}
        for r in (first,) + readers:
            check(S.apply(h, r), want[r], "value", "%s after the candidates (first: %s)" % (r, first), worst)
        h.close()
        report("n = %d %s, first %s" % (n, options, first), worst, len(readers) + 1)


# ---- failure paths ---------------------------------------------------------------------------------------------------------
FAR = 30.0  # lattice spacing in units of ~40 length scales: exp(-FAR^2 / (2 l^2)) is exactly 0, K is block diagonal


def _lattice(k0, k):
    i = np.arange(k0, k0 + k)
    return FAR * np.stack([i % 8, (i // 8) % 8, i // 64], axis=1).astype(float)


@pytest.mark.parametrize("beyond_capacity,sparse_owner", [(False, 300), (True, 100)], ids=["in_place", "new_buffers"])
def test_failed_append_leaves_every_family_as_found(beyond_capacity, sparse_owner):
    """The recipe of test_failed_append_leaves_the_reused_handle_as_found -- Scaled(Normal) at scale 1, no noise on the
    dense factor (UniformNoise at ThetaNoise = 0, which Absorb accepts) and an exact duplicate of an absorbed row: the
    Schur complement is exactly 0 -- in three dimensions: 12 absorbed rows on a lattice too wide for the kernel to
    couple, rows 0 and 1 moved close so that the factor is not the identity.  Outputs, a basis and the other families'
    data are set and observed at their own log thetas (asserted: replay's rule), every reader has run and every family's
    returns values (the sparse workspace's owner: SparseObserve in place, SparseMultiObserve beyond the capacity); after
    the refused Append every reader returns the bits it returned just before."""
    from gogp_amd.gp import GP, FactorizeError
    h = S.Handle(300, GP(S.D, kernel.Scaled(kernel.Normal), S.NOISE, device=0))
    assert h.P == 3
    X0 = _lattice(0, 12)
    X0[1] = X0[0] + [0.3, 0.2, 0.1]
    y0 = np.cos(np.arange(12.0))
    for w in S.origin_sequence("Laplace", sparse_owner)[:-3]:  # the other families
        assert all(S.kind_of(o) == "value" for _, o in S.apply(h, w)), w
    h.g.ThetaSimil, h.g.ThetaNoise = [1.0, 0.7], [0.0]
    h.g.Absorb(X0, y0)
    for w in ("SetOutputs2", "SetBasis2"):
        assert all(S.kind_of(o) == "value" for _, o in S.apply(h, w)), w
    before = {r: S.apply(h, r) for r in S.READER_NAMES}
    values = [r for r in S.READER_NAMES if all(S.kind_of(o) == "value" for _, o in before[r])]
    # all but Gradient (Absorb's factor), the Laplace readers (a regression factor) and the sparse flavour that does not
    # own the workspace
    refused = {"Gradient", "LaplaceGradient", "LaplaceMode", "LaplaceProduce", "SparseMulti" if sparse_owner == 300 else "Sparse"}
    assert set(values) == set(S.READER_NAMES) - refused, sorted(set(S.READER_NAMES) - set(values))
    if beyond_capacity:  # 12 + 301 rows: past the 256 the buffers were allocated for; the duplicate of row 5 comes last
        Xa, ya, pivot = np.concatenate([_lattice(12, 300), X0[5:6]]), np.concatenate([np.linspace(-1, 1, 300), y0[5:6]]), 312
    else:
        Xa, ya, pivot = X0[5:6], y0[5:6], 12
    with pytest.raises(FactorizeError) as ei:
        h.g.Append(Xa, ya)
    assert ei.value.pivot == pivot and h.rows() == 12 and len(h.g.Y) == 12
    worst = {}
    for r in S.READER_NAMES:
        check(S.apply(h, r), before[r], None, "%s after the refused Append" % r, worst)
    h.close()
    report("refused Append", worst, len(S.READER_NAMES))


def test_unconverged_laplace_observe_leaves_the_other_families_as_found():
    """laplace_max_iter = 1: LaplaceObserve raises ConvergenceError with the last iterate stored.  Afterwards the
    regression readers are refused (LaplaceObserve "drops the regression state"), the Laplace readers work on the stored
    iterate, and the sparse, CG, Vecchia and batch readers return their earlier bits; all of it equals a handle that went
    the same way without a reader in between."""
    from gogp_amd.gp import ConvergenceError
    n, seq = 300, S.origin_sequence("ObservePlain", 300)

    def fail(h):
        h.g.set_option("laplace_max_iter", 1)
        h.g.X, h.g.Y = h.c.X, h.c.counts
        with pytest.raises(ConvergenceError) as ei:
            h.g.LaplaceObserve(h.x("poisson"), "poisson")
        assert ei.value.code == _lib.GOGP_ENOCONV and np.isfinite(ei.value.lml)
        return ei.value.lml

    t = S.replay(n, seq)
    lml_t = fail(t)
    want = {r: S.apply(t, r) for r in S.READER_NAMES}
    t.close()
    h = S.replay(n, seq)
    before = {r: S.apply(h, r) for r in S.READER_NAMES}
    assert fail(h) == lml_t
    model = S.model_after(seq + ["LaplacePoisson"])
    worst = {}
    for r in S.READER_NAMES:
        got = S.apply(h, r)
        check(got, want[r], lambda label, r=r: S.expect(model, r, label), "%s after the unconverged LaplaceObserve" % r, worst)
        if r in ("Sparse", "SparseMulti", "SelectInducing", "CG", "Vecchia", "Batch"):
            check(got, before[r], None, "%s against its bits before" % r, worst)
    h.close()
    report("unconverged LaplaceObserve", worst, len(S.READER_NAMES))


def test_basis_produce_without_a_basis_is_refused_like_its_siblings():
    """No basis set: BasisProduce takes an m x 0 Hz to the library, which answers GOGP_ESTATE as BasisLML does."""
    from gogp_amd.gp import GogpError
    h = S.replay(300, ["XY+Observe"])
    for call in (h.g.BasisLML, lambda: h.g.BasisProduce(h.c.Z[5], np.zeros((5, 0)))):
        with pytest.raises(GogpError) as ei:
            call()
        assert ei.value.code == _lib.GOGP_ESTATE
    h.close()


# ---- closing the chain: the fresh twin against the numpy references -------------------------------------------------------
def _vals(n, origin, reader):
    out = twin(n, S.origin_sequence(origin, n), reader)
    assert all(S.kind_of(o) == "value" for _, o in out), (origin, reader, [(l, S.kind_of(o)) for l, o in out])
    return {label: o[1] for label, o in out}


def _close(got, want, tag):
    got, want = np.asarray(got, float), np.asarray(want, float)
    print("%s: %.3e of the rtol 1e-6 + atol 1e-8 criterion" % (tag, (np.abs(got - want) / (1e-8 + 1e-6 * np.abs(want))).max()))
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8, err_msg=tag)


@pytest.fixture(scope="module")
def dense_ref():
    """The dense reference at the Observe origin, n = 300: K = k + s2 I + diag(v) at THETA["observe1"]."""
    c = S.inputs(300)
    ref = NV.Ref(S.D, S.SIMIL, c.X, c.y, c.v)
    ref.observe(S.LOG["observe1"])
    return c, ref


def test_twin_against_the_dense_references(dense_ref):
    c, ref = dense_ref
    v = lambda r: _vals(300, "Observe", r)  # noqa: E731
    lml = v("LML")
    NV.assert_lml(float(lml["LML"][0][0]), ref.lml, "LML")
    _close(lml["Alpha"][0], ref.alpha, "Alpha")
    _close(lml["L"][0], ref.L, "L")
    _close(lml["L_rows"][0], ref.L[[0, 299]], "L_rows")
    _close(lml["L_diag"][0], np.diag(ref.L), "L_diag")
    for name, m in (("Produce5", 5), ("Produce130", 130)):
        for got, want, what in zip(v(name)["Produce"], ref.produce(c.Z[m]), ("mu", "sigma")):
            _close(got, want, "%s %s" % (name, what))
    mu, cov = ref.produce(c.Z[130], cov=True)
    for got, want, what in zip(v("ProduceCovariance")["ProduceCovariance"], (mu, cov), ("mu", "cov")):
        _close(got, want, "ProduceCovariance %s" % what)
    mu65, cov65 = ref.produce(c.Z[65], cov=True)
    C = np.linalg.cholesky(cov65 + S.WR.DIAG_ADD * np.eye(65))
    _close(v("Sample")["Sample"][0], mu65[None, :] + c.xi @ C.T, "Sample")
    NV.assert_gradient(v("Gradient")["Gradient"][0], ref.grad, "Gradient")
    NV.assert_gradient(v("NoiseVariancesGradient")["NoiseVariancesGradient"][0], ref.dv, "NoiseVariancesGradient")
    _close(v("NoiseVariances")["NoiseVariances"][0], c.v, "NoiseVariances")
    mu_l, sg_l, lp_l, g_l = LR.closed_form(ref.K, c.y, ref.dK)
    loo = v("LOO")
    for got, want, what in zip(loo["LOO"], (mu_l, sg_l, lp_l), ("mu", "sigma", "logp")):
        _close(got, want, "LOO %s" % what)
    _close(loo["LOOScore"][0], lp_l.sum(), "LOOScore")
    NV.assert_gradient(v("LOOGradient")["LOOGradient"][0], g_l, "LOOGradient")
    start = S.blocks(300, S.BLOCK)
    mu_b, sg_b, lp_b, g_b = BC.closed_form(ref.K, c.y, start, ref.dK)
    bcv = v("BlockCV")
    for got, want, what in zip(bcv["BlockCV"], (mu_b, sg_b, lp_b), ("mu", "sigma", "logp")):
        _close(got, want, "BlockCV %s" % what)
    _close(bcv["BlockCVScore"][0], lp_b.sum(), "BlockCVScore")
    NV.assert_gradient(v("BlockCVGradient")["BlockCVGradient"][0], g_b, "BlockCVGradient")


def test_twin_against_the_multi_output_and_basis_references(dense_ref):
    c, ref = dense_ref
    v = lambda r: _vals(300, "Observe", r)  # noqa: E731
    Z = c.Z[33]
    Ks = ref._cross(c.X, Z)
    mu0, sigma0 = ref.produce(Z)
    Y = MO.outputs(c.X, 2)
    A, lml, grad = MO.dense(ref.K, Y, ref.dK)
    got = v("MultiLML")
    _close(got["MultiLML"][0], lml.sum(), "MultiLML total")
    _close(got["MultiLML"][1], lml, "MultiLML")
    _close(got["MultiAlpha"][0], A, "MultiAlpha")
    NV.assert_gradient(v("MultiGradient")["MultiGradient"][0], grad, "MultiGradient")
    mp = v("MultiProduce")["MultiProduce"]
    _close(mp[0], Ks.T @ A, "MultiProduce mu")
    _close(mp[1], sigma0, "MultiProduce sigma")
    H, Hz = c.H(c.X, 2), c.H(Z, 2)
    d = BR.dense(ref.K, c.y, H, ref.dK)
    print("cond(H^T K^-1 H) = %.3e" % d["condA"])
    got = v("BasisLML")
    _close(got["BasisLML"][0], d["lml"], "BasisLML")
    _close(got["BasisBeta"][0], d["beta"], "BasisBeta")
    _close(got["BasisBeta"][1], d["cov"], "BasisBeta cov")
    _close(got["BasisAlpha"][0], d["alpha"], "BasisAlpha")
    NV.assert_gradient(v("BasisGradient")["BasisGradient"][0], d["grad"], "BasisGradient")
    prior = sigma0 ** 2 + (np.linalg.solve(ref.L, Ks) ** 2).sum(0)
    mu_b, sigma_b, _, _ = BR.produce_dense(ref.K, Ks, prior, d, Hz)
    bp = v("BasisProduce")["BasisProduce"]
    _close(bp[0], mu_b, "BasisProduce mu")
    _close(bp[1], sigma_b, "BasisProduce sigma")


def test_twin_against_the_references_without_variances():
    """ProduceGradient (its reference takes one noise level), the candidates and the batch, which do not take variances:
    at the ObservePlain origin."""
    c = S.inputs(300)
    th = S.THETA["observe1"]
    pg = _vals(300, "ObservePlain", "ProduceGradient")["ProduceGradient"]
    mu, sigma, dmu, dsigma = PG.reference(S.D, S.SIMIL, th[:2], c.X, c.y, c.Z[33], noise_var=th[2] ** 2)
    _close(pg[0], mu, "ProduceGradient mu")
    _close(pg[1], sigma, "ProduceGradient sigma")
    PG.assert_derivative(pg[2], dmu, "ProduceGradient dmu")
    PG.assert_derivative(pg[3], dsigma, "ProduceGradient dsigma")
    cand = _vals(300, "ObservePlain", "Candidates")
    ref = NV.Ref(S.D, S.SIMIL, c.X, c.y)
    for k, x in enumerate(S.LOG["candidates"]):
        want = ref.observe(x)
        for label in ("candidates", "candidates_again"):
            lmls, grads, status = cand[label]
            assert not status.any()
            NV.assert_lml(lmls[k], want, "%s %d" % (label, k))
            NV.assert_gradient(grads[k], ref.grad, "%s %d gradient" % (label, k))
    bt = _vals(300, "ObservePlain", "Batch")
    Zs = [c.Z[5], c.Z[5][:2], c.Z[5][1:]]
    for i, (o, k) in enumerate(S.BATCH_MEMBERS):
        r = NV.Ref(S.D, S.SIMIL, c.Xb[o:o + k], c.yb[o:o + k])
        want = r.observe(S.LOG["batch"][i])
        lmls, grads, status = bt["batch_observe_gradient"]
        assert not status.any()
        NV.assert_lml(lmls[i], want, "batch %d" % i)
        NV.assert_gradient(grads[i], r.grad, "batch %d gradient" % i)
        out = bt["batch_produce"]  # lmls, k mus, k sigmas, status
        NV.assert_lml(out[0][i], want, "batch_produce %d" % i)
        mu_r, sg_r = r.produce(Zs[i])
        _close(out[1 + i], mu_r, "batch_produce %d mu" % i)
        _close(out[1 + 3 + i], sg_r, "batch_produce %d sigma" % i)
        if i < 2:
            full = bt["batch_observe_full_gradient"]  # lmls, 2 gradients, status
            NV.assert_lml(full[0][i], want, "batch_observe_full_gradient %d" % i)
            NV.assert_gradient(full[1 + i][:3], r.grad, "batch_observe_full_gradient %d" % i)
            pf = bt["batch_produce_full"]  # lmls, 2 mus, 2 sigmas, status
            _close(pf[1 + i], mu_r, "batch_produce_full %d mu" % i)
            _close(pf[1 + 2 + i], sg_r, "batch_produce_full %d sigma" % i)


@pytest.mark.parametrize("lik", ["poisson"])
def test_twin_against_the_laplace_reference(lik):
    c = S.inputs(300)
    x = S.LOG[lik]
    fit, grad = LP.reference(LP.POISSON, S.D, S.SIMIL, x, c.X, c.counts)
    assert fit.converged
    NV.assert_gradient(_vals(300, "Laplace", "LaplaceGradient")["LaplaceGradient"][0], grad, "LaplaceGradient")
    f, a, its = _vals(300, "Laplace", "LaplaceMode")["LaplaceMode"]
    _close(f, fit.f, "LaplaceMode f")
    _close(a, fit.a, "LaplaceMode a")
    assert abs(int(its[0]) - fit.iterations) <= 1
    Ks, prior = LP.cross(S.D, S.SIMIL, x, c.X, c.Z[33])
    for got, want, what in zip(_vals(300, "Laplace", "LaplaceProduce")["LaplaceProduce"], LP.predict(LP.POISSON, fit, Ks, prior),
                               ("mu", "sigma", "mean")):
        _close(got, want, "LaplaceProduce %s" % what)


def test_twin_against_the_sparse_references():
    """SparseGradient / SparseProduce (owner of the workspace at n = 300) and their multi-output forms (at n = 100) at
    the default jitter 1e-8; tests/test_handle_state_cpu.py holds cond(Kuu + eps I) of these inducing points down."""
    c = S.inputs(300)
    eps = 1e-8
    sp = _vals(300, "Observe", "Sparse")
    F, grad, st = SR.reference(S.D, S.SIMIL, S.LOG["sparse"], c.Xsp, c.ysp, c.U, eps)
    NV.assert_gradient(sp["SparseGradient"][0], grad, "SparseGradient")
    NV.assert_gradient(sp["SparseGradientInducing"][0], grad, "SparseGradientInducing")
    for got, want, what in zip(sp["SparseProduce"], SR.produce(S.D, S.SIMIL, S.LOG["sparse"], st, c.U, c.Z[33]), ("mu", "sigma")):
        _close(got, want, "SparseProduce %s" % what)
    sm = _vals(100, "Observe", "SparseMulti")
    total, bounds, gm, dU, stm = SM.reference(S.D, S.SIMIL, S.LOG["sparse_multi"], c.Xsp, c.Ysp, c.U, eps)
    NV.assert_gradient(sm["SparseMultiGradient"][0], gm, "SparseMultiGradient")
    PG.assert_derivative(sm["SparseMultiGradientInducing"][1], dU, "SparseMultiGradientInducing dU")
    for got, want, what in zip(sm["SparseMultiProduce"], SM.produce(S.D, S.SIMIL, S.LOG["sparse_multi"], stm, c.U, c.Z[33]),
                               ("mu", "sigma")):
        _close(got, want, "SparseMultiProduce %s" % what)


def test_twin_against_dense_solves_of_the_cg_and_vecchia_data():
    """CGAlpha, CGProduce and CGSolveColumns solve K^ to tol = 1e-8: against numpy's dense solve within cond tol of the
    solution's norm (cg_ref.alpha_bound's floor), mu and sigma at rtol = 1e-6.  Vecchia with m = 8 is an approximation of
    its own: VecchiaTerms' log densities sum to a valid density, checked against the dense conditionals term by term."""
    c = S.inputs(300)
    ref = NV.Ref(S.D, S.SIMIL, c.Xcg, c.ycg, c.vcg)
    ref.observe(S.LOG["cg"])
    cond = np.linalg.cond(ref.K)
    cg = _vals(300, "Observe", "CG")
    err = np.linalg.norm(cg["CGAlpha"][0] - ref.alpha)
    floor = (cond * 1e-8 + cond * 300 * 2.0 ** -53) * np.linalg.norm(ref.alpha)
    print("CG: cond %.3e, |alpha - dense| %.3e, floor %.3e" % (cond, err, floor))
    assert err <= floor
    mu, sigma = ref.produce(c.Z[5])
    assert np.abs(cg["CGProduce"][0] - mu).max() <= floor * np.abs(ref._cross(c.Xcg, c.Z[5])).sum(0).max()
    np.testing.assert_allclose(cg["CGProduce"][1], sigma, rtol=1e-5)
    S_cols = cg["CGSolveColumns"][0]
    want = np.linalg.solve(ref.K, c.Bcg.T).T
    assert np.linalg.norm(S_cols - want) <= (cond * 1e-8 + cond * 300 * 2.0 ** -53) * np.linalg.norm(want)
    # Vecchia: term i is the dense conditional of row i on the rows its table names
    vc = _vals(300, "Observe", "Vecchia")
    table = vc["VecchiaNeighbourTable"][0]
    rv = NV.Ref(S.D, S.SIMIL, c.Xvc, c.yvc)
    K = rv.gram(S.LOG["vecchia"])
    mu_t, s_t, logp_t = vc["VecchiaTerms"]
    want = np.zeros((300, 3))
    for i in range(300):
        nb = table[i][table[i] >= 0]
        kc = K[np.ix_(nb, nb)]
        w = np.linalg.solve(kc, K[nb, i]) if len(nb) else np.zeros(0)
        m = w @ c.yvc[nb]
        s2 = K[i, i] - w @ K[nb, i]
        want[i] = m, np.sqrt(s2), -0.5 * np.log(2 * np.pi * s2) - 0.5 * (c.yvc[i] - m) ** 2 / s2
    _close(mu_t, want[:, 0], "VecchiaTerms mu")
    _close(s_t, want[:, 1], "VecchiaTerms s")
    _close(logp_t, want[:, 2], "VecchiaTerms logp")
    # ... the forecasts are the dense conditionals on the rows of the tables, which are those of the host search
    np.testing.assert_array_equal(table, VT.nearest(c.Xvc, S.VECCHIA_M))
    np.testing.assert_array_equal(vc["VecchiaNeighbours"][0], VT.nearest(c.Xvc[:50], 5, c.lengths2))
    for label, Z, tz in (("VecchiaProduceNearest", c.Z[33], vc["VecchiaProduceNearest"][2]),
                         ("VecchiaProduce", c.Z[5], VT.nearest_to(c.Xvc, c.Z[5], S.VECCHIA_M))):
        np.testing.assert_array_equal(tz, VT.nearest_to(c.Xvc, Z, S.VECCHIA_M))
        Ks = rv._cross(c.Xvc, Z)
        want = np.zeros((len(Z), 2))
        for j in range(len(Z)):
            nb = tz[j][tz[j] >= 0]
            w = np.linalg.solve(K[np.ix_(nb, nb)], Ks[nb, j])
            want[j] = w @ c.yvc[nb], np.sqrt(rv._cross(Z[j:j + 1], Z[j:j + 1])[0, 0] - w @ Ks[nb, j])
        _close(vc[label][0], want[:, 0], label + " mu")
        _close(vc[label][1], want[:, 1], label + " sigma")
    # ... and the gradient is the sum over the terms of d [LML(c + i) - LML(c)] / d log theta
    grad = np.zeros(3)
    for i in range(300):
        nb = table[i][table[i] >= 0]
        for rows, sign in ((np.append(nb, i), 1.0), (nb, -1.0)):
            if len(rows):
                r = NV.Ref(S.D, S.SIMIL, c.Xvc[rows], c.yvc[rows])
                r.observe(S.LOG["vecchia"])
                grad += sign * r.grad
    NV.assert_gradient(vc["VecchiaGradient"][0], grad, "VecchiaGradient")


def test_twin_against_the_estimator_and_the_selection_references():
    """CGGradient is an estimate from 4 probes: against cg_lml_ref.estimate running the same estimator on the same normals
    (numpy.random.default_rng(3), as GP.CGObserve documents), margin 8 x |its float64 run - its long-double run| plus the
    floor (cond tol + cond N u) max |grad| of the solves, the rule of tests/test_cg_lml_gpu.py.  SelectInducing: the picks
    of select_inducing_ref.greedy, integer for integer, pivots and trace at rtol = 1e-6."""
    c = S.inputs(300)
    th, x = S.THETA["cg"], S.LOG["cg"]
    ref = NV.Ref(S.D, S.SIMIL, c.Xcg, c.ycg, c.vcg)
    _, dK = ref.gram(x, want_grad=True)
    # k(X, X) itself, its diagonal exactly the scale: the pivoted Cholesky's first pick is a tie that rounding must not break
    K = ref._cross(np.array(c.Xcg), np.array(c.Xcg))
    d = th[2] ** 2 + c.vcg
    Kh = K + np.diag(d)
    kp = GR.kp_from_desc(kernel.build_desc(S.D, S.SIMIL, S.NOISE), th[:2], th[2:])
    p = dict(D=S.D, N=S.CG_N, simil=S.SIMIL, kp=kp, X=np.array(c.Xcg), y=np.array(c.ycg), v=np.array(c.vcg), K=K, Kh=Kh, d=d)
    Xi = np.random.default_rng(3).standard_normal((S.CG_PROBES, S.CG_N + S.CG_RANK))
    g = {}
    for mode in ("f64", "ld"):
        e = CL.estimate(p, S.CG_RANK, 1e-8, Xi, piv_tol=1e-8, mode=mode)
        assert e["converged"].all() and e["rank_used"] == S.CG_RANK
        g[mode] = np.array([0.5 * float((e["W"] * dk).sum()) for dk in dK])
    cond = np.linalg.cond(Kh)
    allowed = 8 * np.abs(g["f64"] - g["ld"]).max() + (cond * 1e-8 + cond * S.CG_N * 2.0 ** -53) * np.abs(g["f64"]).max()
    got = _vals(300, "Observe", "CG")["CGGradient"][0]
    print("CGGradient %s, reference %s: max |difference| %.3e, allowed %.3e" % (got, g["f64"], np.abs(got - g["f64"]).max(), allowed))
    assert np.abs(got - g["f64"]).max() <= allowed
    idx, U, pivots, trace = _vals(300, "Observe", "SelectInducing")["SelectInducing"]
    piv, pv, _, _, tr = SI.greedy(SI.dense(S.D, S.SIMIL, S.THETA["select"][:2], c.Xsp), 8, 1e-8)
    np.testing.assert_array_equal(idx, piv)
    np.testing.assert_array_equal(U, c.Xsp[piv])
    _close(pivots, pv, "SelectInducing pivots")
    _close(trace, tr, "SelectInducing trace")
