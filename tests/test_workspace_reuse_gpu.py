"""One fp64 handle that lives through growth and reuse of every grow-on-demand workspace and of the set of N-sized
buffers (handle.h: Workspace, NBufs), each result compared with the same call on a FRESH handle in the same state
(Absorb of the same rows at the same theta).  Every other GPU test uses a fresh handle per call.

Inputs: D = 3, Scaled(Normal) + UniformNoise at theta = (1.0, 0.7 | 0.1), the rows of __graft_entry__.smoke(); n = 300 is
two 256-panels, the second ragged.  The sequence (STEPS): Produce m = 5 (few-point route), ProduceCovariance 130,
ProduceGradient 33, Sample 65 x 2, Produce 130 (tile route: the M buffers regrow), ProduceCovariance 5 (workspace larger
than needed), Append 10 (in place), Append 300 (crosses 512 and exceeds the capacity: a new set of N buffers), Produce 5,
ProduceGradient 33, Remove {0, 255, 256, 600} (npad stays 768), Remove 200 more (npad 768 -> 512), ProduceCovariance
130, Sample 65.

Tolerances: those of the calls' own tests against the oracle -- Produce, ProduceCovariance, Sample and the mu / sigma of
ProduceGradient rtol = 1e-6, atol = 1e-8; a derivative array within 1e-6 of its largest component
(produce_grad_ref.assert_derivative); LML, Alpha and L after Append / Remove append_ref.assert_state.  The fresh handle
reaches its factor by Absorb, the long-lived one by the update: they agree to that tolerance, not bitwise.  The first
six steps run on the same factor bits (both handles absorbed the same 300 rows): bitwise equality there.
test_the_inputs_are_well_conditioned (no GPU) runs the numpy restatements of tests/append_ref.py, tests/remove_ref.py
and tests/produce_cov_ref.py on these rows: they pass the same tolerances against the dense reference, so the rows and
theta leave the comparison room (cond(K) = 3.9e4 at n = 610, cond(cov + diag_add I) = 1.6 at m = 65).

Failure path: with UniformNoise no appended row can make K + noise^2 I indefinite, so the rollback runs on a second
long-lived handle with the kernel of tests/test_append_gpu.py::test_rollback_is_exact (Normal, ConstantNoise(0), a
duplicate of an absorbed point), after the same kinds of calls: once in place (one row) and once beyond the capacity
(300 well separated rows and the duplicate: the new set of N buffers is freed again).  The next Produce and
ProduceCovariance equal, bitwise, the ones taken just before."""
import numpy as np
import pytest

import append_ref as A
import produce_cov_ref as PC
import produce_grad_ref as PG
import remove_ref as R
from gogp_amd import _lib, kernel

D, N0, NROWS = 3, 300, 610
SIMIL, NOISE = kernel.Scaled(kernel.Normal), kernel.UniformNoise
TS, TN = [1.0, 0.7], [0.1]
DIAG_ADD = TN[0] ** 2  # Sample draws noisy observations, as tests/test_produce_covariance_gpu.py
GONE_4 = (0, 255, 256, 600)
GONE_200 = tuple(sorted(int(i) for i in np.random.default_rng(3).choice(NROWS - len(GONE_4), 200, replace=False)))
STEPS = [("produce", 5), ("pcov", 130), ("pgrad", 33), ("sample", 65), ("produce", 130), ("pcov", 5),
         ("append", 10), ("append", 300), ("produce", 5), ("pgrad", 33), ("remove", GONE_4), ("remove", GONE_200),
         ("pcov", 130), ("sample", 65)]
SAME_FACTOR_BITS = 6  # the steps before the first Append


def inputs():
    """(X, y) of all 610 rows, the test points by m, the normals of Sample."""
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (NROWS, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=NROWS)
    Z = {m: rng.uniform(0, 1, (m, D)) for m in (5, 33, 65, 130)}
    return X, y, Z, rng.standard_normal((2, 65))


def new_gp():
    from gogp_amd.gp import GP
    return GP(D, SIMIL, NOISE, ThetaSimil=TS, ThetaNoise=TN, device=0)


def run_step(g, step, rows, X, y, Z, xi):
    """One step on g, whose observations are X[rows]: (the call's outputs, the rows afterwards)."""
    what, arg = step
    if what == "produce":
        return g.Produce(Z[arg]), rows
    if what == "pcov":
        return g.ProduceCovariance(Z[arg]), rows
    if what == "pgrad":
        return g.ProduceGradient(Z[arg]), rows
    if what == "sample":
        return (g.Sample(Z[arg], xi=xi, diag_add=DIAG_ADD),), rows
    if what == "append":
        new = np.arange(rows.max() + 1, rows.max() + 1 + arg)
        g.Append(X[new], y[new])
        rows = np.concatenate([rows, new])
    else:
        g.Remove(arg)
        rows = rows[R.kept_of(len(rows), arg)]
    assert int(_lib.lib().gogp_n(g._h)) == len(rows)
    return (g.LML(), g.Alpha, g.L), rows


def fresh_twin(step, rows_before, rows_after, X, y, Z, xi):
    """The same call on a fresh handle in the same state; after Append / Remove the state Absorb of the rows leaves."""
    g = new_gp()
    if step[0] in ("append", "remove"):
        g.Absorb(X[rows_after], y[rows_after])
        out = (g.LML(), g.Alpha, g.L)
    else:
        g.Absorb(X[rows_before], y[rows_before])
        out = run_step(g, step, rows_before, X, y, Z, xi)[0]
    g.close()
    return out


def assert_close(step, got, want, tag):
    what = step[0]
    if what in ("append", "remove"):
        A.assert_state(*got, *want, tag)
    elif what == "pgrad":
        np.testing.assert_allclose(got[0], want[0], rtol=1e-6, atol=1e-8, err_msg=tag)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-6, atol=1e-8, err_msg=tag)
        PG.assert_derivative(got[2], want[2], tag + " dmu")
        PG.assert_derivative(got[3], want[3], tag + " dsigma")
    else:
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-8, err_msg=tag)


@pytest.mark.gpu
def test_one_handle_through_growth_and_reuse():
    X, y, Z, xi = inputs()
    g = new_gp()
    rows = np.arange(N0)
    g.Absorb(X[rows], y[rows])
    for i, step in enumerate(STEPS):
        tag = "step %d %s %s" % (i, step[0], step[1] if np.isscalar(step[1]) else len(step[1]))
        got, rows_after = run_step(g, step, rows, X, y, Z, xi)
        want = fresh_twin(step, rows, rows_after, X, y, Z, xi)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            a, b = np.asarray(a), np.asarray(b)
            print("%s: max |long-lived - fresh| = %.3e (largest entry %.3e)" % (tag, np.abs(a - b).max(), np.abs(b).max()))
        if i < SAME_FACTOR_BITS:
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b, err_msg=tag)
        else:
            assert_close(step, got, want, tag)
        rows = rows_after
    assert len(rows) == NROWS - len(GONE_4) - len(GONE_200)
    np.testing.assert_array_equal(g.X, X[rows])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beyond_capacity", [False, True], ids=["in_place", "new_buffers"])
def test_failed_append_leaves_the_reused_handle_as_found(beyond_capacity):
    from gogp_amd.gp import GP, FactorizeError
    g = GP(1, kernel.Normal, kernel.ConstantNoise(0.0), ThetaSimil=[1.0], device=0)
    g.Absorb([[0.0], [1.0]], [1.0, 0.0])
    Zs = np.array([[0.25], [0.5], [1.5]])
    Zc = np.linspace(0.1, 1.4, 70)[:, None]
    g.Produce(Zs)  # the workspaces have lived: few-point route, covariance, gradient, samples, tile route
    g.ProduceCovariance(Zc)
    g.ProduceGradient(Zs)
    g.Sample(Zs, xi=np.ones((2, 3)), diag_add=0.5)
    g.Produce(Zc)
    before = g.Produce(Zs) + g.ProduceCovariance(Zc) + (g.L, g.Alpha, g.LML())
    if beyond_capacity:  # 2 + 301 rows: past the 256 the buffers were allocated for; the duplicate of x = 0 comes last
        far = 3.0 + 2.5 * np.arange(300)
        Xa, ya, pivot = np.concatenate([far, [0.0]])[:, None], np.concatenate([np.linspace(-1, 1, 300), [1.0]]), 302
    else:
        Xa, ya, pivot = np.array([[0.0]]), np.array([1.0]), 2
    with pytest.raises(FactorizeError) as ei:
        g.Append(Xa, ya)
    assert ei.value.pivot == pivot
    assert len(g.Y) == 2 and int(_lib.lib().gogp_n(g._h)) == 2
    after = g.Produce(Zs) + g.ProduceCovariance(Zc) + (g.L, g.Alpha, g.LML())
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    g.close()


def test_the_inputs_are_well_conditioned():
    """The numpy restatements of the updates on the sequence's rows against the dense reference, at the tolerances the
    GPU comparison uses (no GPU)."""
    X, y, Z, xi = inputs()

    def dense(rows):
        K = PC.grams(D, SIMIL, TS, X[rows], Z[130], TN[0] ** 2)[0]
        L = np.linalg.cholesky(K)
        al = np.linalg.solve(L.T, np.linalg.solve(L, y[rows]))
        return K, L, al, -0.5 * len(rows) * np.log(2 * np.pi) - np.log(np.diag(L)).sum() - 0.5 * y[rows] @ al

    rows = np.arange(N0 + 310)
    K, L_o, al_o, lml_o = dense(rows)
    print("cond(K) at n = %d: %.3e" % (len(rows), np.linalg.cond(K)))
    L, al, lml = A.block_append(K[:N0 + 10, :N0 + 10], y[:N0 + 10], N0)  # Append 10, then Append 300
    L, al, lml = A.block_append(K, y, N0 + 10)
    A.assert_state(lml, al, L, lml_o, al_o, L_o, "append")
    for gone in (GONE_4, GONE_200):
        L, al, lml = R.state_after_remove(L, y[rows], gone)
        rows = rows[R.kept_of(len(rows), gone)]
        K, L_o, al_o, lml_o = dense(rows)
        A.assert_state(lml, al, L, lml_o, al_o, L_o, "remove %d" % len(gone))
    # the forecast from the updated factor against the dense reference of the rows that are left
    mu_o, cov_o = PC.reference(D, SIMIL, TS, X[rows], y[rows], Z[130], noise_var=TN[0] ** 2)
    Ks = PC.grams(D, SIMIL, TS, X[rows], Z[130], TN[0] ** 2)[1]
    V = np.linalg.solve(L, Ks)
    cov = PC.grams(D, SIMIL, TS, X[rows], Z[130], TN[0] ** 2)[2] - V.T @ V
    np.testing.assert_allclose(Ks.T @ al, mu_o, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(cov, cov_o, rtol=1e-6, atol=1e-8)
    m = 65
    S = cov[:m, :m] + DIAG_ADD * np.eye(m)
    print("cond(cov + diag_add I) at m = %d: %.3e" % (m, np.linalg.cond(S)))
    assert np.linalg.cond(S) < 1e4
