"""The generated sequences of tests/test_handle_state_gpu.py, the classification of GP's public surface, the twin recipe
and the conditioning of the inputs (no GPU).

Conditioning: the numpy references that close the chain on the GPU are run here, on the same rows, thetas, blocks and
counts, against a second statement of the same quantity -- a long-double Cholesky solve, the leave-out refits of
loo_ref.brute_force and blockcv_ref.brute_force, the unwhitened sparse bound -- at the tolerances the GPU comparison
uses, so that those tolerances are not what hides a wrong handle.  cond(K) is printed for n = 300 and n = 100."""
import inspect
import re

import numpy as np
import pytest

import basis_ref as BR
import blockcv_ref as BC
import handle_state_ref as S
import laplace_ref as LP
import loo_ref as LR
import multi_output_ref as MO
import noise_variances_ref as NV
import sparse_ref as SR
from gogp_amd.gp import GP

LD = np.longdouble


# ---- coverage of the generated sequences -----------------------------------------------------------------------------------
def test_every_ordered_pair_of_readers_occurs_on_every_origin():
    triples = S.pair_triples()
    R, O = len(S.READER_NAMES), len(S.ORIGIN_NAMES)
    assert len(triples) == len(set(triples)) == O * len(S.SIZES) * R * R
    assert set(triples) == {(o, n, a, b) for o in S.ORIGIN_NAMES for n in S.SIZES for a in S.READER_NAMES for b in S.READER_NAMES}
    assert len(S.pair_cases()) == O * len(S.SIZES) * R
    assert {"Observe", "Absorb", "Append", "Remove", "Laplace"} <= set(S.ORIGIN_NAMES) and set(S.SIZES) == {300, 100}
    print("%d (origin, n, A, B) cases in %d tests" % (len(triples), len(S.pair_cases())))


def test_every_reader_meets_every_writer():
    quads = S.writer_quadruples()
    R, W = len(S.READER_NAMES), len(S.WRITER_NAMES)
    assert len(quads) == len(set(quads)) == len(S.WRITER_ORIGINS) * W * R * R
    assert {(a, w) for _, a, w, _ in quads} == {(a, w) for a in S.READER_NAMES for w in S.WRITER_NAMES}
    assert S.WRITER_ORIGINS == ["Observe", "Laplace"]
    # the writers the origins are built from and the writers of the cases are all the writers there are
    built = {w for o in S.ORIGIN_NAMES for n in S.SIZES for w in S.origin_sequence(o, n)}
    assert built | set(S.WRITER_NAMES) == set(S.WRITERS)
    print("%d (origin, A, W, B) cases in %d tests" % (len(quads), len(S.writer_cases())))


def test_the_vocabulary_holds_the_calls_it_was_written_for():
    for r in ("LML", "Produce5", "Produce130", "ProduceGradient", "ProduceCovariance", "Sample", "Gradient", "LOO", "LOOGradient",
              "BlockCV", "BlockCVGradient", "MultiLML", "MultiGradient", "MultiProduce", "BasisLML", "BasisGradient",
              "BasisProduce", "NoiseVariancesGradient", "LaplaceGradient", "LaplaceMode", "LaplaceProduce", "Candidates",
              "Batch", "Sparse", "SparseMulti", "CG", "Vecchia"):
        assert r in S.READERS, r
    for w in ("XY300to100+Observe", "XY100to300+Observe", "SetNoiseVariances2", "SetOutputs3", "SetBasis3", "Observe1",
              "Observe2", "Absorb", "Append", "Remove", "restore", "LaplacePoisson", "LaplaceBernoulli", "gradient_precision32",
              "gradient_precision32and64", "SetSparse+SparseObserve", "SetSparseOutputs+SparseMultiObserve", "SetCG+CGObserve",
              "SetVecchiaNearest+VecchiaObserve"):
        assert w in S.WRITER_NAMES, w
    # every observe has a log theta of its own
    rows = [tuple(r) for v in S.THETA.values() for r in np.atleast_2d(np.array(v, float))]
    assert len(rows) == len(set(rows))
    c = S.inputs(300)
    assert len(c.Xa) == 10 and len(c.X) == 300 and len(S.inputs(100).X) == 100 and len(c.Xs) == 100
    assert len(c.Xsp) == 300 and len(c.U) == 32 and len(c.Xcg) == 300 and len(c.Xvc) == 300


# ---- classification of the public surface ----------------------------------------------------------------------------------
HOST_ONLY = {"gogp_destroy", "gogp_graph_info", "gogp_profile_enable", "gogp_profile_read", "gogp_profile_read_launches",
             "gogp_profile_read_aux"}


def test_every_public_method_of_gp_is_classified():
    public = {name for name in vars(GP) if not name.startswith("_")}
    used = {m for methods, _ in S.READERS.values() for m in methods} | {m for w in S.WRITERS.values() for m in w[0]}
    assert used <= public, used - public
    assert not used & set(S.NOT_STATE)
    missing = public - used - set(S.NOT_STATE)
    assert not missing, "neither in the vocabulary nor in NOT_STATE: %s" % sorted(missing)
    assert set(S.NOT_STATE) <= public
    for name, reason in S.NOT_STATE.items():
        assert reason and "\n" not in reason
        calls = set(re.findall(r"gogp_\w+", inspect.getsource(getattr(GP, name))))
        assert calls and calls <= HOST_ONLY, (name, calls)  # no entry point that reads or writes a device buffer


# ---- the twin recipe -------------------------------------------------------------------------------------------------------
def test_twin_drops_readers_and_keeps_writers_in_order():
    assert S.twin_sequence(["Observe1", "Gradient", "LOO", "SetOutputs3", "MultiLML", "Observe2", "Produce5"]) == \
        ["Observe1", "SetOutputs3", "Observe2"]
    assert S.twin_sequence(["Gradient", "Candidates"]) == []
    assert S.twin_sequence(["gradient_precision32", "Gradient", "gradient_precision32and64"]) == \
        ["gradient_precision32", "gradient_precision32and64"]


def test_a_data_setter_drops_the_setters_before_it():
    seq = ["SetCG+CGObserve", "XY+Observe", "SetNoiseVariances", "Observe1", "SetOutputs2", "gradient_precision32", "LML",
           "XY300to100+Observe", "SetBasis3"]
    assert S.twin_sequence(seq) == ["SetCG+CGObserve", "gradient_precision32", "XY300to100+Observe", "SetBasis3"]
    # ... of its own scope only: the sparse, CG, Vecchia and batch data stay, and so do options
    assert S.twin_sequence(["SetSparse+SparseObserve", "SetSparseOutputs+SparseMultiObserve", "Absorb", "CGSolve",
                            "SetSparseGreedy+SparseObserve"]) == ["Absorb", "CGSolve", "SetSparseGreedy+SparseObserve"]
    assert S.twin_sequence(["SetVecchiaNearest+VecchiaObserve", "VecchiaReneighbour+VecchiaObserve",
                            "SetVecchia+VecchiaObserve"]) == ["SetVecchia+VecchiaObserve"]
    for o in S.ORIGIN_NAMES:
        for n in S.SIZES:
            seq = S.origin_sequence(o, n)
            assert S.twin_sequence(seq) == seq  # an origin holds nothing that is replaced again
    # the writers that build a state must succeed on the twin; the call under test (the last `free`) may be refused
    assert S.twin_plan(["XY+Observe", "LOO", "SetOutputs2", "Append"], free=1) == \
        [("XY+Observe", True), ("SetOutputs2", True), ("Append", False)]
    assert S.twin_plan(["XY+Observe", "SetOutputs2", "Absorb"], free=1) == [("Absorb", False)]
    assert all(must for _, must in S.twin_plan(S.origin_sequence("Remove", 100)))


def test_the_table_of_expected_outcomes():
    E = S.EXPECT
    assert len(E) == len(S.ORIGIN_NAMES) * len(S.SIZES) * len(S.READER_NAMES) and set(E.values()) == {"value", "ESTATE", "EARG"}
    assert E[("Absorb", 300, "Gradient")] == "ESTATE" and E[("Observe", 300, "Gradient")] == "value"
    for r in ("LML", "Produce5", "Gradient", "LOO", "BlockCV", "MultiLML", "BasisLML", "NoiseVariancesGradient", "Sample"):
        assert E[("Laplace", 300, r)] == "ESTATE"
    for o in ("Observe", "ObservePlain", "Absorb", "Append", "Remove"):
        for r in ("LaplaceGradient", "LaplaceMode", "LaplaceProduce"):
            assert E[(o, 100, r)] == "ESTATE"
    assert E[("Laplace", 300, "LaplaceGradient")] == "value" and E[("Laplace", 300, "Candidates")] == "value"
    assert E[("Observe", 300, "Candidates")] == "EARG" and E[("ObservePlain", 300, "Candidates")] == "value"
    assert E[("Observe", 300, "Sparse")] == "value" and E[("Observe", 100, "SparseMulti")] == "value"
    m = S.Model()
    assert S.expect(m, "MultiLML") == S.expect(m, "BasisLML") == "ESTATE"  # no outputs, no basis
    m = S.model_after(["XY+Observe", "SetOutputs2", "SetBasis2", "Absorb"])
    assert S.expect(m, "MultiLML") == S.expect(m, "BasisLML") == "ESTATE" and S.expect(m, "Produce5") == "value"
    m = S.model_after(["XY+Observe", "gradient_precision32"])
    assert S.expect(m, "LOO") == "EARG" and S.expect(m, "Gradient") == "value"
    # the two steps that differ from the rest of their call
    m = S.model_after(["LaplacePoisson", "gradient_precision32"])
    assert S.expect(m, "LaplaceMode") == "EARG" and S.expect(m, "LaplaceMode", "LaplaceMode") == "value"
    m = S.model_after(["SetVecchia+VecchiaObserve"])
    assert S.expect(m, "Vecchia", "VecchiaProduceNearest") == "ESTATE" and S.expect(m, "Vecchia", "VecchiaProduce") == "value"
    m = S.model_after(["SetVecchia+VecchiaObserve", "VecchiaReneighbour+VecchiaObserve"])
    assert S.expect(m, "Vecchia", "VecchiaProduceNearest") == "value"


# ---- conditioning of the inputs ----------------------------------------------------------------------------------------------
def chol_solve_ld(K, B):
    """(L, K^-1 B) by a Cholesky factorisation and two substitutions in numpy.longdouble."""
    A = np.array(K, dtype=LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = np.array(B, dtype=LD).reshape(n, -1)
    for j in range(n):
        Z[j] = (Z[j] - L[j, :j] @ Z[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Z[j] = (Z[j] - L[j + 1:, j] @ Z[j + 1:]) / L[j, j]
    return L, Z.reshape(np.shape(B))


def _close(got, want, tag):
    got, want = np.asarray(got, float), np.asarray(want, float)
    print("%s: %.3e of the rtol 1e-6 + atol 1e-8 criterion" % (tag, (np.abs(got - want) / (1e-8 + 1e-6 * np.abs(want))).max()))
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8, err_msg=tag)


@pytest.mark.parametrize("n", S.SIZES)
def test_the_inputs_are_well_conditioned(n):
    c = S.inputs(n)
    ref = NV.Ref(S.D, S.SIMIL, c.X, c.y, c.v)
    for name in ("observe1", "observe2", "absorb", "restore"):
        for v in (c.v, None):
            K = NV.Ref(S.D, S.SIMIL, c.X, c.y, v).gram(S.LOG[name])
            cond = np.linalg.cond(K)
            print("cond(K) at n = %d, theta %s, %s variances: %.3e" % (n, name, "with" if v is not None else "without", cond))
            assert cond < NV.COND_MAX
    ref.observe(S.LOG["observe1"])
    L, sol = chol_solve_ld(ref.K, np.stack([c.y, *MO.outputs(c.X, 2).T, *c.H(c.X, 2).T], axis=1))
    alpha = sol[:, 0]
    lml = -0.5 * n * LD(np.log(2 * np.pi)) - np.log(np.diag(L)).sum() - 0.5 * (c.y.astype(LD) @ alpha)
    NV.assert_lml(ref.lml, float(lml), "LML")
    _close(ref.alpha, alpha, "Alpha")
    _close(ref.L, L, "L")
    # the gradient's weight matrix, LOO and BlockCV from the long-double inverse and from the refits
    Kinv = chol_solve_ld(ref.K, np.eye(n))[1]
    W = np.outer(alpha, alpha) - Kinv
    NV.assert_gradient(ref.grad, [float(0.5 * (W * d).sum()) for d in ref.dK], "Gradient")
    NV.assert_gradient(ref.dv, np.asarray(0.5 * np.diag(W), float), "NoiseVariancesGradient")
    mu, sigma, logp, _ = LR.closed_form(ref.K, c.y, ref.dK)
    for got, want, what in zip((mu, sigma, logp), LR.brute_force(ref.K, c.y), ("mu", "sigma", "logp")):
        _close(got, want, "LOO %s" % what)
    start = S.blocks(n, S.BLOCK)
    mu, sigma, logp, _ = BC.closed_form(ref.K, c.y, start, ref.dK)
    for got, want, what in zip((mu, sigma, logp), BC.brute_force(ref.K, c.y, start), ("mu", "sigma", "logp")):
        _close(got, want, "BlockCV %s" % what)
    # the outputs' and the basis' solutions
    A, lml_t, _ = MO.dense(ref.K, MO.outputs(c.X, 2), ref.dK)
    _close(A, sol[:, 1:3], "MultiAlpha")
    d = BR.dense(ref.K, c.y, c.H(c.X, 2), ref.dK)
    print("cond(H^T K^-1 H) = %.3e" % d["condA"])
    assert d["condA"] < 1e6  # (the bound of tests/test_basis_cpu.py)
    _close(d["W"], sol[:, 3:5], "K^-1 H")
    # the forecast and the draws
    mu65, cov65 = ref.produce(c.Z[65], cov=True)
    condS = np.linalg.cond(cov65 + S.WR.DIAG_ADD * np.eye(65))
    print("cond(cov + diag_add I) at m = 65: %.3e" % condS)
    assert condS < 1e4


@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lik,key", [(LP.POISSON, "poisson"), (LP.BERNOULLI, "bernoulli")])
def test_newton_converges_on_the_counts(lik, key, n):
    c = S.inputs(n)
    y = c.counts if lik == LP.POISSON else c.zero_one
    assert LP.valid(lik, y) and y.any() and (lik == LP.POISSON or not y.all())
    fit, grad = LP.reference(lik, S.D, S.SIMIL, S.LOG[key], c.X, y)
    print("%s n = %d: %d Newton steps, cond(B) = %.3e" % (key, n, fit.iterations, np.linalg.cond(fit.B)))
    assert fit.converged and fit.iterations <= 50 and np.linalg.cond(fit.B) <= 1e5
    # ... and one step does not (test_unconverged_laplace_observe_leaves_the_other_families_as_found)
    assert not LP.mode(lik, LP.gram(S.D, S.SIMIL, S.LOG[key], c.X), y, max_iter=1).converged


def test_the_other_families_data_are_well_conditioned():
    c = S.inputs(300)
    eps = 1e-8
    F, grad, st = SR.reference(S.D, S.SIMIL, S.LOG["sparse"], c.Xsp, c.ysp, c.U, eps)
    cond = np.linalg.cond(st.Kuu + eps * np.eye(len(c.U)))
    direct = SR.direct_bound(S.D, S.SIMIL, S.LOG["sparse"], c.Xsp, c.ysp, c.U, eps)
    print("sparse: cond(Kuu + eps I) = %.3e, bound %.12e, unwhitened %.12e" % (cond, F, direct))
    assert 300 * cond * np.finfo(float).eps < 1e-8  # the rule of tests/test_sparse_gpu.py
    assert abs(F - direct) <= 1e-8 * abs(direct)
    for key, X, v in (("cg", c.Xcg, c.vcg), ("vecchia", c.Xvc, None), ("cg_solve", c.Xcg, c.vcg)):
        cond = np.linalg.cond(NV.Ref(S.D, S.SIMIL, X, np.zeros(len(X)), v).gram(S.LOG[key]))
        print("%s: cond(K) = %.3e" % (key, cond))
        assert cond < NV.COND_MAX
    for i, (o, k) in enumerate(S.BATCH_MEMBERS):
        cond = np.linalg.cond(NV.Ref(S.D, S.SIMIL, c.Xb[o:o + k], c.yb[o:o + k]).gram(S.LOG["batch"][i]))
        print("batch member %d: cond(K) = %.3e" % (i, cond))
        assert cond < NV.COND_MAX
