"""What one gogp_handle logically holds, the calls that act on it, and the twin of a sequence of calls: shared by
tests/test_handle_state_gpu.py (every family against every family on ONE handle) and tests/test_handle_state_cpu.py
(coverage of the generated sequences, classification of GP's public surface, conditioning of the inputs).

Vocabulary.  A WRITER defines state; a READER returns results and must change nothing a later call can see.  Both are
named calls that group the GP methods that belong together (READERS and WRITERS list them per call); a call returns a list of
(label, outcome), an outcome being ("value", arrays) or ("error", status code): a refusal is an outcome like any other.

Twin.  For a sequence of calls the twin is a fresh GP on which only the sequence's writers are replayed, in order, and
then the one call under test (twin_sequence).  A writer that replaces a family's data (DATA_SETTERS) makes every earlier
writer of that family's scope superfluous, so the twin drops them: what such a writer leaves behind may not depend on
what it replaced -- not on a capacity, not on a flag, not on a parameter block left on the device.  Options are never
dropped.  Because the twin runs the same launches on the same inputs, the comparison is bitwise.  A writer that builds a
state must succeed, on the handle and on the twin (replay asserts it); only the call under test may be refused.

State model.  Model holds what the documents say a handle holds after a writer -- which factor (none, Observe's, one
that Gradient refuses, a Laplace fit), whether variances, outputs and a basis are set, the gradient's precision, which
sparse observe owns the shared workspace -- and expect(model, reader) is "value", "ESTATE" or "EARG" by the docstrings of
gogp_amd/gp.py and INTEGRATION.md, not by running the code:
  * LML / Alpha / L, Produce, ProduceGradient, ProduceCovariance, Sample, LOO, BlockCV, NoiseVariancesGradient need a
    regression factor (Absorb, Observe, Append, Remove, restore); Gradient needs Observe's (GP.Gradient: "Gradient
    before Observe");
  * LaplaceObserve "drops the regression state", and a regression factor, SetNoiseVariances or new data drop the fit;
  * Multi* need outputs, Basis* a basis; Absorb, Append, Remove and assigning X / Y drop both (SetOutputs, SetBasis);
  * observe_gradient_candidates and the batch calls leave "the GP's own state" alone; the candidates path and
    LaplaceObserve "do not take" noise variances (SetNoiseVariances): GOGP_EARG;
  * gradient_precision = 32 is refused while variances are set, and with it the calls that read an fp64 K^-1 (LOO,
    BlockCV, NoiseVariancesGradient, Multi*, Basis*, SetNoiseVariances) and LaplaceObserve / LaplaceGradient /
    LaplaceProduce are refused with GOGP_EARG; LaplaceMode still copies out a stored mode (GP.set_option);
  * VecchiaProduceNearest without lengths takes those of the resident table, and is refused where the caller brought
    the table (GP.VecchiaProduceNearest);
  * the two sparse observes share one workspace: the last one owns it, the other flavour's gradient and forecast are
    refused until it observes again (GP.SparseObserve, GP.SparseMultiObserve).

Inputs: D = 3, Scaled(Matern52) + UniformNoise, the rows of test_workspace_reuse_gpu.inputs(); n = 300 (two 256-panels,
the second ragged) and n = 100 (the one-launch `tiny` factorisation); BlockCV blocks(n, 25); sparse N = 300, M = 32;
CG N = 300, rank 16, 4 probes; Vecchia N = 300, m = 8; a batch of three members.  Every observe has a log theta of its
own (THETA), so that a call which leaves its parameters in the handle shows up in the next family's numbers."""
import dataclasses

import numpy as np

import laplace_ref as LP
import multi_output_ref as MO
import noise_variances_ref as NV
import test_workspace_reuse_gpu as WR
from gogp_amd import _lib, basis, kernel
from gogp_amd import vecchia as VT
from gogp_amd.gp import GP, GogpError, blocks

D = 3
SIMIL, NOISE = kernel.Scaled(kernel.Matern52), kernel.UniformNoise
SIZES = (300, 100)
BLOCK = 25
SPARSE_N, SPARSE_M, CG_N, CG_RANK, CG_PROBES, VECCHIA_N, VECCHIA_M = 300, 32, 300, 16, 4, 300, 8
ESTATE, EARG = _lib.GOGP_ESTATE, _lib.GOGP_EARG

#: natural parameters [scale, length | noise std], one set per observe of the vocabulary
THETA = {
    "observe1": [1.0, 0.7, 0.1], "observe2": [1.3, 0.5, 0.15], "absorb": [0.9, 0.6, 0.12], "restore": [1.1, 0.65, 0.14],
    "poisson": [0.8, 0.9, 0.2], "bernoulli": [1.1, 0.8, 0.25],
    "candidates": [[1.2, 0.65, 0.11], [0.95, 0.75, 0.13]],
    "batch": [[1.05, 0.55, 0.14], [0.9, 0.8, 0.12], [1.15, 0.6, 0.16]],
    "sparse": [1.15, 0.62, 0.17], "sparse_multi": [0.85, 0.8, 0.18], "select": [1.0, 0.45, 0.1],
    "cg": [1.25, 0.7, 0.2], "cg_solve": [1.05, 0.75, 0.22], "vecchia": [0.9, 0.5, 0.19],
}
LOG = {k: np.log(np.array(v, dtype=float)) for k, v in THETA.items()}
BATCH_MEMBERS = [(0, 20), (10, 30), (25, 35)]
REMOVE_INNER = (7, 50)  # Remove takes these, row 0 and the last row


class Inputs:
    """Everything the calls read, computed once per n and read only."""

    def __init__(self, n):
        self.n = n
        X, y, Z, xi = WR.inputs()
        self.Xall, self.yall, self.Z, self.xi = X, y, Z, xi
        self.X, self.y = X[:n], y[:n]
        self.X2, self.y2 = X[300:300 + n], y[300:300 + n]  # other rows of the same count (a change of n and back)
        self.Xs, self.ys = X[100:100 + 100], y[100:200]    # the 100 rows of the change of n
        self.Xa, self.ya, self.va = X[n:n + 10], y[n:n + 10], NV.variances(10, seed=5)
        self.v, self.v2 = NV.variances(n), NV.variances(n, seed=12)
        self.counts = LP.draw(LP.POISSON, LP.gram(D, SIMIL, LOG["poisson"], self.X))
        self.zero_one = LP.draw(LP.BERNOULLI, LP.gram(D, SIMIL, LOG["bernoulli"], self.X))
        self.Xsp, self.ysp = X[310:310 + SPARSE_N], y[310:310 + SPARSE_N]
        self.U, self.U2 = self.Xsp[:SPARSE_M], self.Xsp[SPARSE_M:2 * SPARSE_M]
        self.Ysp = MO.outputs(self.Xsp, 2, seed=11)
        self.Xcg, self.ycg, self.vcg = X[150:150 + CG_N], y[150:150 + CG_N], NV.variances(CG_N, seed=21)
        self.Bcg = np.stack([np.cos(3.0 * self.Xcg[:, 0]), self.Xcg[:, 1] - 0.5])
        self.Xvc, self.yvc = X[200:200 + VECCHIA_N], y[200:200 + VECCHIA_N]
        self.lengths2 = [0.5, 1.0, 2.0]
        self.Xb, self.yb = X[:60], y[:60]
        self.fc, self.fs = np.array([0.5]), np.array([0.5])  # the frame of the polynomial basis: x_0 in [0, 1]
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def H(self, X, p):
        return basis.polynomial(X, p - 1, [0], self.fc, self.fs) if p else np.zeros((len(X), 0))


_INPUTS = {}


def inputs(n):
    if n not in _INPUTS:
        _INPUTS[n] = Inputs(n)
    return _INPUTS[n]


class Handle:
    """A GP and what the calls have to remember beside it."""

    def __init__(self, n, gp=None, basis_symm=None):
        self.c = inputs(n)
        self.g = gp if gp is not None else GP(D, SIMIL, NOISE, device=0)
        if basis_symm is not None:  # the route of the Basis* calls pinned (None: the default, by whether K^-1 is there)
            self.g.set_option("basis_symm", basis_symm)
        self.log = []
        self.P = len(self.g.ThetaSimil) + len(self.g.ThetaNoise)  # hyperparameters: 3 with the vocabulary's kernel
        self.p = 0        # columns of the last SetBasis (BasisProduce takes m x p rows)
        self.keep = []    # device tensors of set_data_device

    def rows(self):
        return int(_lib.lib().gogp_n(self.g._h))

    def x(self, name):
        """log theta of one observe of the vocabulary, cut to the handle's hyperparameters"""
        return np.ascontiguousarray(LOG[name][..., :self.P])

    def close(self):
        self.g.close()
        self.keep.clear()


# ---- outcomes ----------------------------------------------------------------------------------------------------------
def flatten(r):
    """The arrays of a result: tuples, lists and dicts (by sorted key) flattened, scalars as 0-d arrays, None dropped."""
    if r is None:
        return []
    if isinstance(r, dict):
        return [a for k in sorted(r) for a in flatten(r[k])]
    if isinstance(r, (tuple, list)):
        return [a for x in r for a in flatten(x)]
    a = np.asarray(r)
    return [np.ascontiguousarray(a if a.dtype.kind in "iub" else a.astype(np.float64))]


def outcome(thunk):
    try:
        r = thunk()
    except GogpError as e:
        return ("error", int(e.code))
    return ("value", flatten(r))


def run(steps):
    return [(label, outcome(thunk)) for label, thunk in steps]


def _set_theta(g, name):
    g.ThetaSimil, g.ThetaNoise = list(THETA[name][:2]), list(THETA[name][2:])[:len(g.ThetaNoise)]


# ---- readers --------------------------------------------------------------------------------------------------------------
def _r_lml(h):
    g = h.g
    return [("LML", g.LML), ("Alpha", lambda: g.Alpha), ("L", lambda: g.L), ("L_rows", lambda: g.L_rows([0, h.rows() - 1])),
            ("L_diag", g.L_diag)]


def _r_sparse(h):
    g = h.g
    return [("SparseGradient", g.SparseGradient), ("SparseGradientInducing", g.SparseGradientInducing),
            ("SparseProduce", lambda: g.SparseProduce(h.c.Z[33]))]


def _r_sparse_multi(h):
    g = h.g
    return [("SparseMultiGradient", g.SparseMultiGradient), ("SparseMultiGradientInducing", g.SparseMultiGradientInducing),
            ("SparseMultiProduce", lambda: g.SparseMultiProduce(h.c.Z[33]))]


def _r_cg(h):
    g = h.g
    return [("CGGradient", g.CGGradient), ("CGAlpha", g.CGAlpha), ("CGProduce", lambda: g.CGProduce(h.c.Z[5])),
            ("CGSolveColumns", lambda: g.CGSolveColumns(h.c.Bcg))]


def _r_vecchia(h):
    g, c = h.g, h.c
    return [("VecchiaTerms", g.VecchiaTerms), ("VecchiaGradient", g.VecchiaGradient),
            ("VecchiaProduceNearest", lambda: g.VecchiaProduceNearest(c.Z[33], table=True)),
            ("VecchiaProduce", lambda: g.VecchiaProduce(c.Z[5], VT.nearest_to(c.Xvc, c.Z[5], VECCHIA_M))),
            ("VecchiaNeighbourTable", g.VecchiaNeighbourTable),
            ("VecchiaNeighbours", lambda: g.VecchiaNeighbours(c.Xvc[:50], 5, c.lengths2))]


def _r_candidates(h):
    # twice in a row: the second call replays the captured graph
    return [("candidates", lambda: h.g.observe_gradient_candidates(h.x("candidates"))),
            ("candidates_again", lambda: h.g.observe_gradient_candidates(h.x("candidates")))]


def _r_batch(h):
    g, c, xs = h.g, h.c, h.x("batch")
    full = [np.concatenate([xs[i], c.Xb[o:o + k].ravel(), c.yb[o:o + k]]) for i, (o, k) in enumerate(BATCH_MEMBERS[:2])]
    Zs = [c.Z[5], c.Z[5][:2], c.Z[5][1:]]
    return [("batch_observe_gradient", lambda: g.batch_observe_gradient(xs)),
            ("batch_produce", lambda: g.batch_produce(xs, Zs)),
            ("batch_observe_full_gradient", lambda: g.batch_observe_full_gradient(full)),
            ("batch_produce_full", lambda: g.batch_produce_full(full, Zs[:2]))]


#: name -> (the GP methods the call stands for, the steps of the call)
READERS = {
    "LML": (("LML", "Alpha", "L", "L_rows", "L_diag"), _r_lml),
    "Produce5": (("Produce",), lambda h: [("Produce", lambda: h.g.Produce(h.c.Z[5]))]),
    "Produce130": (("Produce",), lambda h: [("Produce", lambda: h.g.Produce(h.c.Z[130]))]),
    "ProduceGradient": (("ProduceGradient",), lambda h: [("ProduceGradient", lambda: h.g.ProduceGradient(h.c.Z[33]))]),
    "ProduceCovariance": (("ProduceCovariance",),
                          lambda h: [("ProduceCovariance", lambda: h.g.ProduceCovariance(h.c.Z[130]))]),
    "Sample": (("Sample",), lambda h: [("Sample", lambda: h.g.Sample(h.c.Z[65], xi=h.c.xi, diag_add=WR.DIAG_ADD))]),
    "Gradient": (("Gradient",), lambda h: [("Gradient", h.g.Gradient)]),
    "LOO": (("LOO", "LOOScore"), lambda h: [("LOO", h.g.LOO), ("LOOScore", h.g.LOOScore)]),
    "LOOGradient": (("LOOGradient",), lambda h: [("LOOGradient", h.g.LOOGradient)]),
    "BlockCV": (("BlockCV", "BlockCVScore"), lambda h: [("BlockCV", lambda: h.g.BlockCV(blocks(h.rows(), BLOCK))),
                                                         ("BlockCVScore", lambda: h.g.BlockCVScore(blocks(h.rows(), BLOCK)))]),
    "BlockCVGradient": (("BlockCVGradient",),
                        lambda h: [("BlockCVGradient", lambda: h.g.BlockCVGradient(blocks(h.rows(), BLOCK)))]),
    "MultiLML": (("MultiLML", "MultiAlpha"), lambda h: [("MultiLML", h.g.MultiLML), ("MultiAlpha", lambda: h.g.MultiAlpha)]),
    "MultiGradient": (("MultiGradient",), lambda h: [("MultiGradient", h.g.MultiGradient)]),
    "MultiProduce": (("MultiProduce",), lambda h: [("MultiProduce", lambda: h.g.MultiProduce(h.c.Z[33]))]),
    "BasisLML": (("BasisLML", "BasisBeta", "BasisAlpha"),
                 lambda h: [("BasisLML", h.g.BasisLML), ("BasisBeta", h.g.BasisBeta), ("BasisAlpha", lambda: h.g.BasisAlpha)]),
    "BasisGradient": (("BasisGradient",), lambda h: [("BasisGradient", h.g.BasisGradient)]),
    "BasisProduce": (("BasisProduce",),
                     lambda h: [("BasisProduce", lambda: h.g.BasisProduce(h.c.Z[33], h.c.H(h.c.Z[33], h.p)))]),
    "NoiseVariances": (("NoiseVariances",), lambda h: [("NoiseVariances", lambda: h.g.NoiseVariances)]),
    "NoiseVariancesGradient": (("NoiseVariancesGradient",), lambda h: [("NoiseVariancesGradient", h.g.NoiseVariancesGradient)]),
    "LaplaceGradient": (("LaplaceGradient",), lambda h: [("LaplaceGradient", h.g.LaplaceGradient)]),
    "LaplaceMode": (("LaplaceMode",), lambda h: [("LaplaceMode", h.g.LaplaceMode)]),
    "LaplaceProduce": (("LaplaceProduce",), lambda h: [("LaplaceProduce", lambda: h.g.LaplaceProduce(h.c.Z[33]))]),
    "Candidates": (("observe_gradient_candidates",), _r_candidates),
    "Batch": (("batch_observe_gradient", "batch_produce", "batch_observe_full_gradient", "batch_produce_full"), _r_batch),
    "Sparse": (("SparseGradient", "SparseGradientInducing", "SparseProduce"), _r_sparse),
    "SparseMulti": (("SparseMultiGradient", "SparseMultiGradientInducing", "SparseMultiProduce"), _r_sparse_multi),
    "SelectInducing": (("SelectInducing",), lambda h: [("SelectInducing", lambda: h.g.SelectInducing(h.x("select"), 8))]),
    "CG": (("CGGradient", "CGAlpha", "CGProduce", "CGSolveColumns"), _r_cg),
    "Vecchia": (("VecchiaTerms", "VecchiaGradient", "VecchiaProduceNearest", "VecchiaProduce", "VecchiaNeighbourTable",
                 "VecchiaNeighbours"), _r_vecchia),
}
READER_NAMES = list(READERS)


# ---- the state model ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Model:
    factor: str = "none"     # none | observe | factor (Absorb, Append, Remove, restore: Gradient refuses) | laplace
    nv: bool = False         # noise variances set
    T: int = 0               # output columns
    p: int = 0               # basis columns
    gp32: bool = False       # gradient_precision = 32
    sparse: str = "none"     # which sparse observe owns the shared workspace: none | single | multi
    sparse_T: int = 0
    table: str = "none"      # who built the Vecchia table: none | device | caller

    def regression(self):
        return self.factor in ("observe", "factor")


def expect(m, reader, label=None):
    """"value", "ESTATE" or "EARG": what every step of the reader -- or its step `label`, where the steps differ -- returns
    on a handle in state m (module docstring)."""
    if label == "LaplaceMode":  # (copies the stored mode: no arithmetic that gradient_precision = 32 could refuse)
        return "value" if m.factor == "laplace" else "ESTATE"
    if label == "VecchiaProduceNearest" and m.table == "caller":  # lengths = None: the table's own, and it has none
        return "ESTATE"
    if reader in ("NoiseVariances", "Batch", "SelectInducing", "CG", "Vecchia"):
        return "value"
    if reader in ("LML", "Produce5", "Produce130", "ProduceGradient", "ProduceCovariance", "Sample"):
        return "value" if m.regression() else "ESTATE"
    if reader == "Gradient":
        return "value" if m.factor == "observe" else "ESTATE"
    if reader in ("LOO", "LOOGradient", "BlockCV", "BlockCVGradient", "NoiseVariancesGradient"):
        return "EARG" if m.gp32 else ("value" if m.regression() else "ESTATE")
    if reader.startswith("Multi"):
        return "EARG" if m.gp32 else ("value" if m.T and m.regression() else "ESTATE")
    if reader.startswith("Basis"):
        return "EARG" if m.gp32 else ("value" if m.p and m.regression() else "ESTATE")
    if reader.startswith("Laplace"):
        return "EARG" if m.gp32 else ("value" if m.factor == "laplace" else "ESTATE")
    if reader == "Candidates":
        return "EARG" if m.nv else "value"
    if reader == "Sparse":
        return "value" if m.sparse == "single" else "ESTATE"
    if reader == "SparseMulti":
        return "value" if m.sparse == "multi" else "ESTATE"
    raise KeyError(reader)


# ---- writers --------------------------------------------------------------------------------------------------------------
# fn(h): the steps; model(m): the state afterwards (in place)
def _new_data(m, factor):
    m.factor, m.nv, m.T, m.p = factor, False, 0, 0


def _w_xy(rows):
    def fn(h):
        c = h.c
        X, y = {"n": (c.X, c.y), "n2": (c.X2, c.y2), "100": (c.Xs, c.ys)}[rows]

        def go():
            h.g.X, h.g.Y = X, y
            return h.g.Observe(h.x("observe1"))
        return [("XY+Observe", go)]
    return fn


def _w_to100to300(h):
    return _w_xy("100")(h) + _w_xy("n2")(h)


def _w_device(h):
    def go():
        import torch
        dX = torch.tensor(np.array(h.c.Xs), dtype=torch.float64, device="cuda:0")
        dy = torch.tensor(np.array(h.c.ys), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        h.keep += [dX, dy]
        h.g.set_data_device(dX.data_ptr(), dy.data_ptr(), len(h.c.ys))
        return h.g.Observe(h.x("observe1"))
    return [("set_data_device+Observe", go)]


def _w_nv(which):
    return lambda h: [("SetNoiseVariances", lambda: h.g.SetNoiseVariances(getattr(h.c, which)[:h.rows()]))]


def _m_nv(m):
    if not m.gp32:
        m.factor, m.nv = "none", True


def _w_outputs(T):
    return lambda h: [("SetOutputs", lambda: h.g.SetOutputs(MO.outputs(h.g.X, T)))]


def _m_outputs(T):
    def model(m):
        if not m.gp32:
            m.T = T
    return model


def _w_basis(p):
    def fn(h):
        def go():
            h.g.SetBasis(h.c.H(h.g.X, p))
            h.p = p
        return [("SetBasis", go)]
    return fn


def _m_basis(p):
    def model(m):
        if not m.gp32:
            m.p = p
    return model


def _w_absorb(h):
    def go():
        _set_theta(h.g, "absorb")
        h.g.Absorb(h.c.X, h.c.y)
    return [("Absorb", go)]


def _w_absorb_v(h):
    def go():
        _set_theta(h.g, "absorb")
        h.g.Absorb(h.c.X, h.c.y, h.c.v)
    return [("Absorb", go)]


def _m_absorb_v(m):
    _new_data(m, "factor")
    m.nv = not m.gp32  # (SetNoiseVariances is refused beside gradient_precision = 32: Absorb then raises after the upload)
    if m.gp32:
        m.factor = "none"


def _w_append(h):
    def go():
        h.g.Append(h.c.Xa, h.c.ya, h.c.va if h.g.NoiseVariances.any() else None)
    return [("Append", go)]


def _w_remove(h):
    def go():
        h.g.Remove((0,) + REMOVE_INNER + (h.rows() - 1,))
    return [("Remove", go)]


def _m_update(m):
    if m.regression():
        m.factor, m.T, m.p = "factor", 0, 0


_RESTORE = {}


def restore_arrays(n):
    """(L, Alpha) of the rows at THETA["restore"], taken once from a handle of their own."""
    if n not in _RESTORE:
        h = Handle(n)
        _set_theta(h.g, "restore")
        h.g.Absorb(h.c.X, h.c.y)
        _RESTORE[n] = (h.g.L, h.g.Alpha)
        h.close()
    return _RESTORE[n]


def _w_restore(h):
    def go():
        L, al = restore_arrays(h.c.n)
        _set_theta(h.g, "restore")
        h.g.restore(L, al)
    return [("restore", go)]


def _m_restore(m):
    m.factor = "factor"


def _w_laplace(lik):
    def fn(h):
        def go():
            h.g.X, h.g.Y = h.c.X, (h.c.counts if lik == "poisson" else h.c.zero_one)
            return h.g.LaplaceObserve(h.x(lik), lik)
        return [("LaplaceObserve", go)]
    return fn


def _m_laplace(m):
    _new_data(m, "none" if m.gp32 else "laplace")


def _w_option(name, values):
    return lambda h: [("%s=%d" % (name, v), (lambda v=v: h.g.set_option(name, v))) for v in values]


def _m_gp32(m):
    if not m.nv:
        m.gp32 = True


def _m_gp32_back(m):
    m.gp32 = False


def _w_sparse(h):
    g, c = h.g, h.c
    return [("SetSparse", lambda: g.SetSparse(c.Xsp, c.ysp, c.U)), ("SparseObserve", lambda: g.SparseObserve(h.x("sparse")))]


def _w_sparse_multi(h):
    g, c = h.g, h.c
    return [("SetSparseOutputs", lambda: g.SetSparseOutputs(c.Ysp)),
            ("SparseMultiObserve", lambda: g.SparseMultiObserve(h.x("sparse_multi")))]


def _w_inducing(h):
    g, c = h.g, h.c
    return [("SetInducing", lambda: g.SetInducing(c.U2)), ("SparseObserve", lambda: g.SparseObserve(h.x("sparse")))]


def _w_greedy(h):
    g, c = h.g, h.c
    return [("SetSparseGreedy", lambda: g.SetSparseGreedy(c.Xsp, c.ysp, SPARSE_M, h.x("select"))),
            ("SparseObserve", lambda: g.SparseObserve(h.x("sparse")))]


def _m_sparse(owner, drop_outputs=False):
    def model(m):
        if drop_outputs:
            m.sparse_T = 0
        if owner == "multi":
            m.sparse_T = 2
        m.sparse = owner
    return model


def _w_cg(h):
    g, c = h.g, h.c
    return [("SetCG", lambda: g.SetCG(c.Xcg, c.ycg, c.vcg)),
            ("CGObserve", lambda: g.CGObserve(h.x("cg"), probes=CG_PROBES, seed=3, rank=CG_RANK))]


def _w_cg_solve(h):
    return [("CGSolve", lambda: h.g.CGSolve(h.x("cg_solve"), rank=CG_RANK))]


def _w_vecchia(h):
    g, c = h.g, h.c
    return [("SetVecchiaNearest", lambda: g.SetVecchiaNearest(c.Xvc, c.yvc, VECCHIA_M)),
            ("VecchiaObserve", lambda: g.VecchiaObserve(h.x("vecchia")))]


def _w_vecchia_host(h):
    g, c = h.g, h.c
    return [("SetVecchia", lambda: g.SetVecchia(c.Xvc, c.yvc, VT.previous(VECCHIA_N, VECCHIA_M))),
            ("VecchiaObserve", lambda: g.VecchiaObserve(h.x("vecchia")))]


def _w_reneighbour(h):
    g, c = h.g, h.c
    return [("VecchiaReneighbour", lambda: g.VecchiaReneighbour(c.lengths2)),
            ("VecchiaObserve", lambda: g.VecchiaObserve(h.x("vecchia")))]


def _w_batch(h):
    return [("set_batch", lambda: h.g.set_batch(h.c.Xb, h.c.yb, BATCH_MEMBERS))]


def _m_none(m):
    pass


def _m_table(who):
    def model(m):
        m.table = who
    return model


def _m_observe(m):
    m.factor = "observe"


#: name -> (the GP methods, scope, the steps, the model's update)
WRITERS = {
    "XY+Observe": (("X", "Y", "Observe"), "dense", _w_xy("n"), lambda m: _new_data(m, "observe")),
    "XY300to100+Observe": (("X", "Y", "Observe"), "dense", _w_xy("100"), lambda m: _new_data(m, "observe")),
    "XY100to300+Observe": (("X", "Y", "Observe"), "dense", _w_to100to300, lambda m: _new_data(m, "observe")),
    "set_data_device+Observe": (("set_data_device", "Observe"), "dense", _w_device, lambda m: _new_data(m, "observe")),
    "SetNoiseVariances": (("SetNoiseVariances",), "dense", _w_nv("v"), _m_nv),
    "SetNoiseVariances2": (("SetNoiseVariances",), "dense", _w_nv("v2"), _m_nv),
    "SetOutputs2": (("SetOutputs",), "dense", _w_outputs(2), _m_outputs(2)),
    "SetOutputs3": (("SetOutputs",), "dense", _w_outputs(3), _m_outputs(3)),
    "SetBasis2": (("SetBasis",), "dense", _w_basis(2), _m_basis(2)),
    "SetBasis3": (("SetBasis",), "dense", _w_basis(3), _m_basis(3)),
    "Observe1": (("Observe",), "dense", lambda h: [("Observe", lambda: h.g.Observe(h.x("observe1")))], _m_observe),
    "Observe2": (("Observe",), "dense", lambda h: [("Observe", lambda: h.g.Observe(h.x("observe2")))], _m_observe),
    "Absorb": (("Absorb",), "dense", _w_absorb, lambda m: _new_data(m, "factor")),
    "AbsorbNoisy": (("Absorb",), "dense", _w_absorb_v, _m_absorb_v),
    "Append": (("Append",), "dense", _w_append, _m_update),
    "Remove": (("Remove",), "dense", _w_remove, _m_update),
    "restore": (("restore",), "dense", _w_restore, _m_restore),
    "LaplacePoisson": (("X", "Y", "LaplaceObserve"), "dense", _w_laplace("poisson"), _m_laplace),
    "LaplaceBernoulli": (("X", "Y", "LaplaceObserve"), "dense", _w_laplace("bernoulli"), _m_laplace),
    "gradient_precision32": (("set_option",), "option", _w_option("gradient_precision", (32,)), _m_gp32),
    "gradient_precision32and64": (("set_option",), "option", _w_option("gradient_precision", (32, 64)), _m_gp32_back),
    "SetSparse+SparseObserve": (("SetSparse", "SparseObserve"), "sparse", _w_sparse, _m_sparse("single", True)),
    "SetSparseOutputs+SparseMultiObserve": (("SetSparseOutputs", "SparseMultiObserve"), "sparse", _w_sparse_multi,
                                            _m_sparse("multi")),
    "SparseObserve": (("SparseObserve",), "sparse", lambda h: [("SparseObserve", lambda: h.g.SparseObserve(h.x("sparse")))],
                      _m_sparse("single")),
    "SetInducing+SparseObserve": (("SetInducing", "SparseObserve"), "sparse", _w_inducing, _m_sparse("single")),
    "SetSparseGreedy+SparseObserve": (("SetSparseGreedy", "SparseObserve"), "sparse", _w_greedy, _m_sparse("single", True)),
    "SetCG+CGObserve": (("SetCG", "CGObserve"), "cg", _w_cg, _m_none),
    "CGSolve": (("CGSolve",), "cg", _w_cg_solve, _m_none),
    "SetVecchiaNearest+VecchiaObserve": (("SetVecchiaNearest", "VecchiaObserve"), "vecchia", _w_vecchia, _m_table("device")),
    "SetVecchia+VecchiaObserve": (("SetVecchia", "VecchiaObserve"), "vecchia", _w_vecchia_host, _m_table("caller")),
    "VecchiaReneighbour+VecchiaObserve": (("VecchiaReneighbour", "VecchiaObserve"), "vecchia", _w_reneighbour, _m_table("device")),
    "set_batch": (("set_batch",), "batch", _w_batch, _m_none),
}
#: the writers that replace their scope's data: the twin drops the scope's earlier writers
DATA_SETTERS = {"XY+Observe", "XY300to100+Observe", "XY100to300+Observe", "set_data_device+Observe", "Absorb", "AbsorbNoisy",
                "LaplacePoisson", "LaplaceBernoulli", "SetSparse+SparseObserve", "SetSparseGreedy+SparseObserve",
                "SetCG+CGObserve", "SetVecchiaNearest+VecchiaObserve", "SetVecchia+VecchiaObserve", "set_batch"}
#: the writers of the writer-after-reader cases (the others build the origins)
WRITER_NAMES = [w for w in WRITERS if w not in ("XY+Observe", "SetNoiseVariances", "SetOutputs2", "SetBasis2", "AbsorbNoisy")]

#: GP's public names that are no call of the vocabulary, each with its reason; none touches a device buffer
NOT_STATE = {
    "close": "destroys the handle: nothing can follow it",
    "graph_info": "reads two host-side diagnostics of the candidates graph",
    "profile_enable": "switches the host-side timers of the launches on or off",
    "profile_read": "reads and resets the host-side timers",
    "profile_read_launches": "reads the host-side launch records",
    "profile_read_aux": "reads one class of host-side timers",
}

_FAMILIES_MULTI_LAST = ["SetSparse+SparseObserve", "SetSparseOutputs+SparseMultiObserve", "SetCG+CGObserve",
                        "SetVecchiaNearest+VecchiaObserve", "set_batch"]
_FAMILIES = _FAMILIES_MULTI_LAST[:2] + ["SparseObserve"] + _FAMILIES_MULTI_LAST[2:]
_TAIL = ["SetOutputs2", "SetBasis2"]
#: origin -> its writers after the other families' (families(n)), in order
ORIGINS = {
    "Observe": ["XY+Observe", "SetNoiseVariances", "Observe1"] + _TAIL,
    "ObservePlain": ["XY+Observe"] + _TAIL,
    "Absorb": ["AbsorbNoisy"] + _TAIL,
    "Append": ["XY+Observe", "SetNoiseVariances", "Observe1", "Append"] + _TAIL,
    "Remove": ["XY+Observe", "SetNoiseVariances", "Observe1", "Remove"] + _TAIL,
    "Laplace": ["LaplacePoisson"] + _TAIL,
}
ORIGIN_NAMES = list(ORIGINS)
WRITER_ORIGINS = ["Observe", "Laplace"]  # of the writer-after-reader cases, at n = 300


def origin_sequence(origin, n):
    """The writers that build an origin.  The sparse workspace has one owner: SparseObserve at n = 300, SparseMultiObserve
    at n = 100, so that both flavours' readers return values somewhere."""
    fam = _FAMILIES if n == 300 else _FAMILIES_MULTI_LAST
    return list(fam) + list(ORIGINS[origin])


def twin_plan(seq, free=0):
    """[(writer, must succeed)] of the twin of a sequence of call names: its writers in order, without the readers and
    without the writers that a later data setter of the same scope replaces.  The last `free` calls of seq are the ones
    under test, which may be refused; every writer before them builds a state and must succeed."""
    out = []
    for i, name in enumerate(seq):
        if name in READERS:
            continue
        scope = WRITERS[name][1]
        if name in DATA_SETTERS:
            out = [(w, must) for w, must in out if WRITERS[w][1] != scope]
        out.append((name, i < len(seq) - free))
    return out


def twin_sequence(seq):
    return [w for w, _ in twin_plan(seq)]


def model_after(seq):
    m = Model()
    for name in seq:
        if name in WRITERS:
            WRITERS[name][3](m)
    return m


def apply(h, name):
    """One call of the vocabulary on the handle: [(label, outcome)]."""
    steps = (READERS[name][1] if name in READERS else WRITERS[name][2])(h)
    return run(steps)


def replay(n, plan, basis_symm=None):
    """A fresh handle after the calls of plan -- names, or (name, must succeed) pairs as twin_plan gives them; a name alone
    must succeed: a writer that builds a state may not fail unseen.  h.log keeps every call's results."""
    h = Handle(n, basis_symm=basis_symm)
    for item in plan:
        name, must = (item, True) if isinstance(item, str) else item
        out = apply(h, name)
        h.log.append((name, out))
        if must:
            bad = [(label, kind_of(o)) for label, o in out if o[0] != "value"]
            assert not bad, "%s while building a state: %s" % (name, bad)
    return h


# ---- the generated cases ---------------------------------------------------------------------------------------------------
def pair_cases():
    """(origin, n, A): one handle each, B looping over every reader with A called again before each."""
    return [(o, n, a) for o in ORIGIN_NAMES for n in SIZES for a in READER_NAMES]


def pair_triples():
    return [(o, n, a, b) for o, n, a in pair_cases() for b in READER_NAMES]


def writer_cases():
    """(origin, W): at n = 300, one handle per reader A -- origin, A, W, then every reader once."""
    return [(o, w) for o in WRITER_ORIGINS for w in WRITER_NAMES]


def writer_quadruples():
    return [(o, a, w, b) for o, w in writer_cases() for a in READER_NAMES for b in READER_NAMES]


EXPECT = {(o, n, r): expect(model_after(origin_sequence(o, n)), r) for o in ORIGIN_NAMES for n in SIZES for r in READER_NAMES}


# ---- comparison -----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def kind_of(out):
    """"value" / "ESTATE" / "EARG" / "error <code>" of one outcome."""
    if out[0] == "value":
        return "value"
    return {ESTATE: "ESTATE", EARG: "EARG"}.get(out[1], "error %d" % out[1])


def largest_difference(got, want):
    """The largest |difference| over the arrays of two value outcomes (inf where shapes differ)."""
    worst = 0.0
    for a, b in zip(got, want):
        if a.shape != b.shape:
            return float("inf")
        if a.size:
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            worst = max(worst, float(np.nanmax(d)) if not np.isnan(d).all() else 0.0)
    return worst


def compare(got, want, tolerant=(), tag=""):
    """Two results of one call, label by label: the same kind of outcome, the same code, the same bits -- or, for the
    labels in `tolerant`, rtol = 1e-6 and atol = 1e-8 (1e-6 of the largest component for a gradient).  Returns the
    largest difference per label, for printing."""
    assert [l for l, _ in got] == [l for l, _ in want], tag
    diffs = {}
    for (label, a), (_, b) in zip(got, want):
        assert kind_of(a) == kind_of(b), "%s %s: %s on this handle, %s on the twin" % (tag, label, kind_of(a), kind_of(b))
        if a[0] != "value":
            continue
        assert len(a[1]) == len(b[1]), (tag, label)
        diffs[label] = largest_difference(a[1], b[1])
        for u, v in zip(a[1], b[1]):
            if label in tolerant:
                if "Gradient" in label or "gradient" in label:
                    assert u.shape == v.shape and np.abs(u - v).max(initial=0.0) <= 1e-6 * np.abs(v).max(initial=0.0), \
                        (tag, label, diffs[label])
                else:
                    np.testing.assert_allclose(u, v, rtol=1e-6, atol=1e-8, err_msg="%s %s" % (tag, label))
            else:
                assert same_bits(u, v), "%s %s: not the twin's bits, max |difference| = %.3e" % (tag, label, diffs[label])
    return diffs
