"""Priors of the reference's case studies, the host-side callers of the GP hot path through
gp.Model (gp/model.go:9-28).  The reference differentiates them with
infergo's tape; here the gradients are written out.  Log-densities as in infergo's ``dist``
package (bitbucket.org/dtolpin/infergo/dist, a dependency of the reference that is not vendored
in /root/reference): Normal.Logp(mu, sigma, x) = -((x-mu)/sigma)^2/2 - log sigma - log(2 pi)/2,
Expon.Logp(lambda, y) = log lambda - lambda y."""
import math

import numpy as np

_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def _normal_logp(mu, sigma, x):
    return -0.5 * ((x - mu) / sigma) ** 2 - math.log(sigma) - _LOG_SQRT_2PI


class HyperPriors:
    """tutorial/hyperpriors/model/model.go:9-44: normal priors on the log-parameters
    [c1, c2, l1, l2, p, s] of trend + seasonality (kernel: tutorial/hyperpriors/kernel/kernel.go);
    the seasonality weight's prior is centred log 2 below the trend weight."""

    def Observe(self, x) -> float:
        x = np.asarray(x, dtype=float)
        c1, c2, l1, l2, p, s = x[:6]
        ll = _normal_logp(-1.0, 1.0, c1)
        ll += _normal_logp(c1 - math.log(2.0), 1.0, c2)
        ll += _normal_logp(0.0, 2.0, l1) + _normal_logp(0.0, 2.0, l2)
        ll += _normal_logp(0.0, 1.0, p) + _normal_logp(0.0, 1.0, s)
        d = c2 - (c1 - math.log(2.0))
        self._grad = np.array([-(c1 + 1.0) + d, -d, -l1 / 4.0, -l2 / 4.0, -p, -s])
        return float(ll)

    def Gradient(self) -> np.ndarray:
        return self._grad


class AnyNoisePriors:
    """tutorial/anynoise/model/model.go:8-50: x = [log c, log l, log s | inputs | outputs] (the full
    Observe form, 1-D inputs).  Normal priors on the three parameters; the LATENT outputs carried
    in x are tied to the noisy outputs memorised at the first call by a Laplacian likelihood,
    Expon.Logp(1/exp(x[s]), |Y_i - x_out_i|)."""

    def __init__(self):
        self.Y = None

    def Observe(self, x) -> float:
        x = np.asarray(x, dtype=float)
        n = (x.size - 3) // 2
        out = x[3 + n:]
        if self.Y is None or len(self.Y) != n:  # first call: memoise the initial outputs
            self.Y = out.copy()
        c, l, s = x[:3]
        ll = _normal_logp(-1.0, 1.0, c) + _normal_logp(0.0, 2.0, l) + _normal_logp(-1.0, 2.0, s)
        lam = 1.0 / math.exp(s)
        dev = self.Y - out
        ll += n * math.log(lam) - lam * np.abs(dev).sum()
        g = np.zeros(x.size)
        g[0] = -(c + 1.0)
        g[1] = -l / 4.0
        g[2] = -(s + 1.0) / 4.0 - n + lam * np.abs(dev).sum()  # d/ds of n log(1/e^s) - |dev|/e^s
        g[3 + n:] = lam * np.sign(dev)                          # d/d out_i of -lam |Y_i - out_i|
        self._grad = g
        return float(ll)

    def Gradient(self) -> np.ndarray:
        return self._grad


class AnyNoiseModel:
    """tutorial/anynoise/main.go:29-44: gp.Model whose gradient w.r.t. the INPUTS is wiped (only the
    hyperparameters and the latent outputs are inferred)."""

    def __init__(self, model):
        self.Model = model
        self.GP = model.GP

    def Observe(self, x) -> float:
        return self.Model.Observe(x)

    def Gradient(self) -> np.ndarray:
        g = np.array(self.Model.Gradient(), dtype=float)
        n = len(self.GP.X)
        return self.edit_gradient(g, _ntheta(self.GP), n, self.GP.NDim)

    @staticmethod
    def edit_gradient(g, p, n, ndim):
        g[p:p + n * ndim] = 0.0
        return g

    def window_objective(self):
        """A fresh host-side objective for one window of the batched harness (tutorial.BATCH): this model's priors,
        not yet memoised, and its edit of the gradient."""
        return WindowObjective(type(self.Model.Priors)(), _ntheta(self.GP), self.GP.NDim, self.edit_gradient)


def _ntheta(gp) -> int:
    return gp._ns + gp._nn if hasattr(gp, "_ns") else gp._P


class WindowObjective:
    """The host side of one forecast window of the batched harness (tutorial.BATCH with OPTINP): what a model
    wrapper around gp.Model adds to the GP's value and gradient at x -- the priors (gp/model.go:17-28) and the
    wrapper's edit of the gradient -- with a priors state of its OWN, because the case studies' priors memoise
    at their first call (the window's start vector).  ``value(x, lml)`` is Model.Observe, ``value_grad(x, lml,
    grad)`` is Model.Observe + the wrapper's Gradient, given the GP's LML and full-form gradient at x."""

    def __init__(self, priors, ntheta, ndim, edit):
        self.Priors, self.ntheta, self.ndim, self.edit = priors, ntheta, ndim, edit

    def value(self, x, lml):
        return lml + self.Priors.Observe(x)

    def value_grad(self, x, lml, grad):
        v = lml + self.Priors.Observe(x)
        pg = np.asarray(self.Priors.Gradient(), dtype=float)
        g = np.array(grad, dtype=float)
        g[:len(pg)] += pg
        n = (len(g) - self.ntheta) // (self.ndim + 1)
        return v, self.edit(g, self.ntheta, n, self.ndim)


class WarpedTimePriors:
    """tutorial/warpedtime/model/model.go:8-60: x = [log c, log l, log s | inputs | outputs] (the full Observe
    form, 1-D inputs).  Normal priors on the three parameters; the inputs may move a little: the relative steps
    (x_{i+1} - x_i) / step_i ~ Normal(1, exp(LogSigma)), with step_i the distances between the inputs at the first
    call of a given length (memoised, :22-40)."""

    def __init__(self, LogSigma: float = math.log(0.5)):
        self.LogSigma = LogSigma
        self.step = None

    def Observe(self, x) -> float:
        x = np.asarray(x, dtype=float)
        n = (x.size - 3) // 2
        inp = x[3:3 + n]
        nstep = max(n - 1, 0)
        if self.step is None or len(self.step) != nstep:  # first call: memoise the initial steps
            self.step = np.diff(inp).copy() if n > 1 else np.zeros(0)
        c, l, s = x[:3]
        ll = _normal_logp(-1.0, 1.0, c) + _normal_logp(0.0, 2.0, l) + _normal_logp(0.5, 1.0, s)
        g = np.zeros(x.size)
        g[0] = -(c + 1.0)
        g[1] = -l / 4.0
        g[2] = -(s - 0.5)
        if nstep:
            sigma = math.exp(self.LogSigma)
            r = np.diff(inp) / self.step
            ll += float((-0.5 * ((r - 1.0) / sigma) ** 2).sum()) - nstep * (self.LogSigma + _LOG_SQRT_2PI)
            dr = -(r - 1.0) / (sigma * sigma) / self.step  # d ll / d (x_{i+1} - x_i)
            g[3 + 1:3 + n] += dr
            g[3:3 + n - 1] -= dr
        self._grad = g
        return float(ll)

    def Gradient(self) -> np.ndarray:
        return self._grad


class WarpedTimeModel:
    """tutorial/warpedtime/main.go:40-56: gp.Model whose gradient w.r.t. the FIRST input and everything from the
    LAST input on (the last input and all outputs) is wiped: the end points stay put, the inner inputs move."""

    def __init__(self, model):
        self.Model = model
        self.GP = model.GP

    def Observe(self, x) -> float:
        return self.Model.Observe(x)

    def Gradient(self) -> np.ndarray:
        g = np.array(self.Model.Gradient(), dtype=float)
        return self.edit_gradient(g, _ntheta(self.GP), len(self.GP.X), self.GP.NDim)

    @staticmethod
    def edit_gradient(g, p, n, ndim):
        if n > 0:  # (:48-53; the reference indexes past the vector without observations)
            g[p] = 0.0
            g[p + n - 1:] = 0.0
        return g

    def window_objective(self):
        pr = self.Model.Priors
        return WindowObjective(type(pr)(pr.LogSigma), _ntheta(self.GP), self.GP.NDim, self.edit_gradient)
