"""Host-side mirror of the reference's ``gp`` package (gp/gp.go, gp/model.go)
over the C ABI of include/gogp_hip.h.

``GP`` keeps the reference's field and method names -- ``NDim, Simil, Noise,
ThetaSimil, ThetaNoise, X, Y, Parallel`` and ``Absorb / LML / Produce / Observe
/ Gradient`` (gp/gp.go:20-38,80,244,258,374,418) -- with the same argument
meaning and the same error behaviour:

  * ``Absorb`` returns normally or raises ``FactorizeError`` where the Go method
    returns ``err`` (gp/gp.go:228-230);
  * ``Observe`` raises where the reference panics (gp/gp.go:398-405);
  * ``Produce`` returns ``(mu, sigma)`` or raises (gp/gp.go:338-340).

All arithmetic runs on the GPU through libgogp_hip.so; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import operator
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .kernel import NoiseKernel, SimilKernel, build_desc


class GogpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("gogp_hip error %d: %s" % (code, msg))
        self.code = code


class FactorizeError(GogpError):
    """gp/gp.go:228-230: Factorize(K) failed, K is not positive definite."""

    def __init__(self, msg: str, pivot: int):
        super().__init__(_lib.GOGP_ENOTPD, msg)
        self.pivot = pivot


class ConditionError(GogpError):
    """gonum's mat.Condition error (cond > 1e16) that gp/gp.go:233-236 returns from Absorb
    and turns into a panic in Observe: K factored, but it is numerically singular.  The state
    (L, Alpha, LML) was stored before the error was reported, as in gonum."""

    def __init__(self, msg: str):
        super().__init__(_lib.GOGP_ECOND, msg)


class ConvergenceError(GogpError):
    """gogp_laplace_observe: Newton's iteration for the mode of the Laplace approximation did not reach the tolerance
    (GOGP_ENOCONV).  The last iterate was stored before the error was reported, as with ConditionError: ``lml`` is its
    approximate log marginal likelihood, and LaplaceGradient / LaplaceMode / LaplaceProduce work on it."""

    def __init__(self, msg: str, lml: float = float("nan")):
        super().__init__(_lib.GOGP_ENOCONV, msg)
        self.lml = lml


#: the likelihoods of GP.LaplaceObserve, by name (enum gogp_lik_kind)
LIKELIHOODS = {"bernoulli": _lib.GOGP_LIK_BERNOULLI_LOGIT, "poisson": _lib.GOGP_LIK_POISSON_LOG}


def _lik(lik) -> int:
    if isinstance(lik, str):
        if lik not in LIKELIHOODS:
            raise ValueError("lik: one of %s" % ", ".join(sorted(LIKELIHOODS)))
        return LIKELIHOODS[lik]
    return int(lik)


def _dp(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _arr(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _starts(start) -> np.ndarray:
    """The F + 1 block starts of the block cross-validation calls as the int64 array the library reads."""
    st = np.ascontiguousarray(np.asarray(start, dtype=np.int64).reshape(-1))
    if st.size < 1:
        raise ValueError("start: F + 1 entries, from 0 to n")
    return st


def blocks(n: int, length: int) -> np.ndarray:
    """``start`` of GP.BlockCV for n rows in consecutive blocks of ``length`` rows, the last one shorter where length
    does not divide n: [0, length, 2 length, ..., n].  n = 0 gives [0]."""
    if n < 0 or length < 1:
        raise ValueError("blocks: n >= 0 and length >= 1")
    return np.append(np.arange(0, n, length, dtype=np.int64), np.int64(n))


class GP:
    """Type GP is the barebone implementation of GP (gp/gp.go:19-38)."""

    def __init__(self, NDim: int, Simil: SimilKernel, Noise: Optional[NoiseKernel] = None,
                 ThetaSimil: Optional[Sequence[float]] = None,
                 ThetaNoise: Optional[Sequence[float]] = None,
                 X=None, Y=None, Parallel: bool = False, device: int = -1, precision: int = 64):
        self.NDim = int(NDim)
        self.Simil = Simil
        self.Noise = Noise
        # gp/gp.go:45-57 defaults(): Noise nil => ConstantNoise(1e-5) (done by
        # build_desc); zero theta vectors when empty
        self._desc = build_desc(self.NDim, Simil, Noise)
        self._ns = Simil.NTheta()
        self._nn = 0 if self._desc.noise_kind == 0 else 1
        self.ThetaSimil: List[float] = list(ThetaSimil) if ThetaSimil is not None else [0.0] * self._ns
        self.ThetaNoise: List[float] = list(ThetaNoise) if ThetaNoise is not None else [0.0] * self._nn
        #: accepted for source compatibility; the device path is always parallel
        self.Parallel = Parallel
        #: HIP device index of the handle (-1: the device current at construction)
        self.device = int(device)
        self._sparse_m = 0  # inducing points of SetSparse
        self._sparse_t = 0  # output columns of SetSparseOutputs
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        rc = L.gogp_create(ctypes.byref(self._desc), int(device), ctypes.byref(self._h))
        if rc != _lib.GOGP_OK:
            msg = L.gogp_last_error(None).decode()
            self._h = ctypes.c_void_p()
            raise GogpError(rc, msg)
        #: 64: fp64 throughout (the reference's arithmetic).  32: the N x N matrices and the
        #: O(N^3) products in fp32 (BASELINE configs[4]); inputs, kernel evaluation, diagonal
        #: blocks, vectors and reductions stay fp64 -- include/gogp_hip.h, option "precision"
        self.precision = int(precision)
        if self.precision != 64:
            self._check(L.gogp_set_option(self._h, b"precision", self.precision))
        events = getattr(Simil, "events", None)
        if events:  # kernel.Events: the discounts of tutorial/events/kernel/kernel.go:14-44 (gogp_set_events)
            ev = np.ascontiguousarray(np.asarray(events, dtype=np.float64).reshape(-1, 3))
            self._check(L.gogp_set_events(self._h, _dp(ev), len(ev), int(Simil.event_axis)))
        self._X = np.zeros((0, self.NDim))
        self._Y = np.zeros((0,))
        self._data_dirty = True
        self._with_obs = False
        self._last_len = self._ns + self._nn
        if X is not None:
            self.X = X
            self.Y = Y if Y is not None else []

    # ---- plumbing ------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().gogp_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc == _lib.GOGP_OK:
            return
        L = _lib.lib()
        msg = L.gogp_last_error(self._h).decode()
        if rc == _lib.GOGP_ENOTPD:
            raise FactorizeError(msg, int(L.gogp_notpd_index(self._h)))
        if rc == _lib.GOGP_ECOND:
            raise ConditionError(msg)
        raise GogpError(rc, msg)

    # ---- data: gp.GP.X / gp.GP.Y (gp/gp.go:27-28) --------------------------------
    @property
    def X(self) -> np.ndarray:
        return self._X

    @X.setter
    def X(self, x):
        self._X = _arr(x).reshape(-1, self.NDim)
        self._data_dirty = True

    @property
    def Y(self) -> np.ndarray:
        return self._Y

    @Y.setter
    def Y(self, y):
        self._Y = _arr(y).reshape(-1)
        self._data_dirty = True

    def _push_data(self):
        if not self._data_dirty:
            return
        if len(self._X) != len(self._Y):
            raise ValueError("len(X) != len(Y)")
        self._check(_lib.lib().gogp_set_data(self._h, _dp(self._X), _dp(self._Y), len(self._Y)))
        self._data_dirty = False

    def set_data_device(self, dX_ptr: int, dy_ptr: int, n: int):
        """Inputs already resident in HBM (device pointers, e.g. torch .data_ptr())."""
        self._check(_lib.lib().gogp_set_data_device(self._h, ctypes.c_void_p(dX_ptr),
                                                    ctypes.c_void_p(dy_ptr), int(n)))
        self._data_dirty = False

    # ---- per-observation noise variances (no reference counterpart: gp.GP has one noise level) ----
    def SetNoiseVariances(self, v) -> None:
        """Known noise variances, one per observation: K = k(X, X) + sigma^2(theta) I + diag(v), every v[i] finite and
        >= 0 (gogp_set_noise_variances).  ``None`` clears them.  Stored results are dropped: Absorb or Observe again
        before Gradient, Produce, LOO ...; every call behind the factorisation then sees the variances.  They belong
        to the data: assigning ``X`` / ``Y`` (and so Absorb(x, y) without ``v``, and the full form of Observe) clears
        them; Append and Remove carry them.  fp64, unsharded handles; the candidates path, the Laplace calls, the
        batches of small GPs and the sparse calls do not take them."""
        if v is None:
            if not self._data_dirty:
                self._check(_lib.lib().gogp_set_noise_variances(self._h, None, 0))
            return
        va = _arr(v).reshape(-1)
        if va.size != len(self._Y):
            raise ValueError("SetNoiseVariances: one variance per observation")
        self._push_data()
        self._check(_lib.lib().gogp_set_noise_variances(self._h, _dp(va), va.size))

    @property
    def NoiseVariances(self) -> np.ndarray:
        """The noise variances the device holds for the current observations (zeros when none are set)."""
        if self._data_dirty:
            return np.zeros(len(self._Y))
        v = np.zeros(int(_lib.lib().gogp_n(self._h)))
        self._check(_lib.lib().gogp_get_noise_variances(self._h, _dp(v)))
        return v

    def NoiseVariancesGradient(self) -> np.ndarray:
        """dLML/dv[i] = 1/2 (Alpha[i]^2 - [K^-1]_ii), n entries, at the parameters and variances of the last Absorb /
        Observe / Append / Remove / restore (gogp_noise_variances_gradient); also with no variances set (the
        derivative at v = 0).  Works wherever LOO works and leaves the process as it found it."""
        dv = np.zeros(int(_lib.lib().gogp_n(self._h)))
        self._check(_lib.lib().gogp_noise_variances_gradient(self._h, _dp(dv)))
        return dv

    # ---- gp.GP.Absorb (gp/gp.go:80-87) -----------------------------------------------
    def Absorb(self, x, y, v=None) -> None:
        """Absorb absorbs observations into the process.  Parameters are taken
        from ThetaSimil / ThetaNoise (natural scale, gp/gp_test.go:29).  ``v``: the observations' noise variances
        (SetNoiseVariances); None: none, also when the previous data had some."""
        self.X, self.Y = x, y
        self._push_data()
        if v is not None:
            self.SetNoiseVariances(v)
        ts = _arr(self.ThetaSimil)
        tn = _arr(self.ThetaNoise) if self._nn else np.zeros(1)
        if ts.size != self._ns:
            raise ValueError("len(ThetaSimil)")
        self._with_obs = False
        self._check(_lib.lib().gogp_absorb(self._h, _dp(ts), _dp(tn)))

    # ---- no reference counterpart (the reference refactorises: tutorial/tutorial.go:118-142) ----
    def Append(self, x, y, v=None) -> None:
        """Append observations to the absorbed ones at the parameters of the last Absorb / Observe / restore
        (gogp_append_noisy): the state Absorb on all observations would leave, without a new factorisation.  An empty
        process absorbs them at ThetaSimil / ThetaNoise.  ``v``: the new observations' noise variances
        (SetNoiseVariances); None: zeros.  With ``v`` on a process without variances the old rows get zeros.  Raises
        FactorizeError (``pivot``: the global index) and leaves the process -- its variances, outputs and basis included
        -- as it was when the enlarged matrix is not positive definite."""
        xa = _arr(x).reshape(-1, self.NDim)
        ya = _arr(y).reshape(-1)
        if len(xa) != len(ya):
            raise ValueError("len(x) != len(y)")
        va = None
        if v is not None:
            va = _arr(v).reshape(-1)
            if len(va) != len(ya):
                raise ValueError("len(v) != len(y)")
        L = _lib.lib()
        if len(self._Y) == 0:
            # an empty process: pending (empty) data first, and the parameters the append is to use
            self._push_data()
            ts = _arr(self.ThetaSimil)
            tn = _arr(self.ThetaNoise) if self._nn else np.zeros(1)
            if ts.size != self._ns:
                raise ValueError("len(ThetaSimil)")
            self._check(L.gogp_absorb(self._h, _dp(ts), _dp(tn)))
        elif self._data_dirty:
            # the device no longer holds X / Y: nothing there to append to
            raise GogpError(_lib.GOGP_ESTATE, "Append: X / Y were assigned since the last Absorb / Observe; Absorb them")
        if len(ya) == 0:
            return
        rc = L.gogp_append_noisy(self._h, _dp(xa), _dp(ya), _dp(va), len(ya))
        if rc in (_lib.GOGP_OK, _lib.GOGP_ECOND):  # stored (GOGP_ECOND: and reported, as Absorb)
            self._X = np.concatenate([self._X.reshape(-1, self.NDim), xa])
            self._Y = np.concatenate([self._Y, ya])
            self._with_obs = False
        self._check(rc)

    def Remove(self, idx) -> None:
        """Remove the observations with the indices ``idx`` (any iterable of ints; sorted here) from the absorbed
        ones (gogp_remove): the state Absorb on the kept rows, in their order, would leave, without a new
        factorisation and at the parameters of the last Absorb / Observe / restore.  The counterpart of Append; with
        it a bounded window slides: ``Remove([0])``, then ``Append(new)``.  Duplicates and indices outside
        ``[0, len(Y))`` raise ValueError before the library is called."""
        ia = sorted(operator.index(i) for i in idx)
        n = len(self._Y)
        if any(i < 0 or i >= n for i in ia):
            raise ValueError("Remove: index out of range")
        if any(a == b for a, b in zip(ia, ia[1:])):
            raise ValueError("Remove: duplicate index")
        if self._data_dirty:
            # the device no longer holds X / Y: nothing there to remove from
            raise GogpError(_lib.GOGP_ESTATE, "Remove: X / Y were assigned since the last Absorb / Observe; Absorb them")
        if not ia:
            return
        arr = np.ascontiguousarray(ia, dtype=np.int64)
        rc = _lib.lib().gogp_remove(self._h, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(arr))
        if rc in (_lib.GOGP_OK, _lib.GOGP_ECOND):  # stored (GOGP_ECOND: and reported, as Absorb)
            keep = np.ones(n, dtype=bool)
            keep[arr] = False
            self._X = np.ascontiguousarray(self._X.reshape(-1, self.NDim)[keep])
            self._Y = np.ascontiguousarray(self._Y[keep])
            self._with_obs = False
        self._check(rc)

    # ---- gp.GP.LML (gp/gp.go:244-253) -----------------------------------------------
    def LML(self) -> float:
        v = ctypes.c_double(0.0)
        self._check(_lib.lib().gogp_lml(self._h, ctypes.byref(v)))
        return v.value

    # ---- gp.GP.Produce (gp/gp.go:258-360) --------------------------------------------
    def Produce(self, x):
        z = _arr(x).reshape(-1, self.NDim)
        m = len(z)
        mu, sigma = np.zeros(m), np.zeros(m)
        if m:
            if self._data_dirty and len(self._Y) == 0:
                self._push_data()
            self._check(_lib.lib().gogp_produce(self._h, _dp(z), m, _dp(mu), _dp(sigma)))
        return mu, sigma

    def ProduceGradient(self, x):
        """Produce and the derivatives of the forecast with respect to the test points:
        (mu, sigma, dmu, dsigma) with dmu[j, d] = d mu_j / d x[j, d] and dsigma[j, d] =
        d sigma_j / d x[j, d], both of shape (m, NDim).  mu and sigma are what Produce(x)
        returns.  No reference counterpart: gp.GP.Produce returns mu and sigma only.  sigma
        is not clamped: a row of dsigma whose sigma^2 is not positive is NaN / inf.  fp64,
        unsharded handles only."""
        z = _arr(x).reshape(-1, self.NDim)
        m = len(z)
        mu, sigma = np.zeros(m), np.zeros(m)
        dmu, dsigma = np.zeros((m, self.NDim)), np.zeros((m, self.NDim))
        if m:
            if self._data_dirty and len(self._Y) == 0:
                self._push_data()
            self._check(_lib.lib().gogp_produce_gradient(self._h, _dp(z), m, _dp(mu), _dp(sigma), _dp(dmu),
                                                         _dp(dsigma)))
        return mu, sigma, dmu, dsigma

    def _test_points(self, x) -> np.ndarray:
        z = _arr(x)
        if z.ndim == 2 and z.shape[1] != self.NDim:
            raise ValueError("test points have %d columns, the GP has NDim = %d" % (z.shape[1], self.NDim))
        return z.reshape(-1, self.NDim)

    def ProduceCovariance(self, x):
        """(mu, cov): Produce's mu and the joint covariance of the latent function at the m test
        points, cov = k(Z, Z) - Kstar^T K^-1 Kstar (m x m, exactly symmetric, no noise term:
        sqrt(diag(cov)) is Produce's sigma to rounding).  No reference counterpart: gp.GP.Produce
        keeps the diagonal only.  At most GOGP_COV_MAX_M points; fp64, unsharded handles only."""
        z = self._test_points(x)
        m = len(z)
        mu, cov = np.zeros(m), np.zeros((m, m))
        if m:
            if self._data_dirty and len(self._Y) == 0:
                self._push_data()
            self._check(_lib.lib().gogp_produce_covariance(self._h, _dp(z), m, _dp(mu), _dp(cov)))
        return mu, cov

    def Sample(self, x, ns: int = 1, rng=None, xi=None, diag_add: float = 0.0) -> np.ndarray:
        """ns joint draws (ns x m) at the m test points: mu + C xi with C the lower Cholesky factor
        of ProduceCovariance(x)'s cov + diag_add I.  diag_add = 0 draws the latent function, the
        noise variance draws noisy observations, a small value is jitter where cov is numerically
        singular.  xi: the standard normals to use (ns x m); drawn on the host from `rng`
        (default np.random.default_rng()) when None.  Raises FactorizeError (pivot = index among
        the test points) when cov + diag_add I is not positive definite."""
        z = self._test_points(x)
        m = len(z)
        if xi is None:
            ns = int(ns)
            if ns < 0:
                raise ValueError("ns < 0")
            xi = (np.random.default_rng() if rng is None else rng).standard_normal((ns, m))
        else:
            xi = _arr(xi)
            if xi.ndim == 1 and m > 0 and xi.size == m:
                xi = xi.reshape(1, m)
            if xi.ndim != 2 or xi.shape[1] != m:
                raise ValueError("xi must have shape (ns, %d), not %r" % (m, xi.shape))
            ns = xi.shape[0]
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        mu, out = np.zeros(m), np.zeros((ns, m))
        if m:
            if self._data_dirty and len(self._Y) == 0:
                self._push_data()
            self._check(_lib.lib().gogp_produce_samples(self._h, _dp(z), m, _dp(xi), ns, float(diag_add), _dp(mu),
                                                        _dp(out)))
        return out

    # ---- gp.GP.Observe (gp/gp.go:374-413) ---------------------------------------------
    def Observe(self, x) -> float:
        """x = log-transformed hyperparameters [| inputs | outputs].  Raises where
        the reference panics.  x itself is not modified (the reference's in-place
        exp/log round trip, gp/gp.go:378-381,408-410, is not reproduced)."""
        xa = _arr(x).reshape(-1)
        P = self._ns + self._nn
        if xa.size < P:
            raise ValueError("len(x)")
        lml = ctypes.c_double(0.0)
        L = _lib.lib()
        if xa.size == P:
            self._push_data()
            self._with_obs = False
            rc = L.gogp_observe(self._h, _dp(xa), xa.size, ctypes.byref(lml))
        else:
            rest = xa.size - P
            n = rest // (self.NDim + 1)
            if n * (self.NDim + 1) != rest:
                raise ValueError("len(x)")  # gp/gp.go:398-400 panic("len(x)")
            rc = L.gogp_observe_full(self._h, _dp(xa), xa.size, ctypes.byref(lml))
            # gp/gp.go:391-396: X, Y are re-sliced from x -- also when the factorisation then
            # fails (the reference panics after the assignment): the device holds these data now
            self._X = xa[P:P + n * self.NDim].reshape(n, self.NDim).copy()
            self._Y = xa[P + n * self.NDim:].copy()
            self._data_dirty = rc != _lib.GOGP_OK  # after a failure: re-upload before the next call
            self._with_obs = rc == _lib.GOGP_OK
        self._check(rc)
        theta = np.exp(xa[:P])
        self.ThetaSimil = list(theta[:self._ns])  # gp/gp.go:384-385
        self.ThetaNoise = list(theta[self._ns:])
        self._last_len = xa.size
        return lml.value

    # ---- gp.GP.Gradient (gp/gp.go:418-499) ---------------------------------------------
    def Gradient(self) -> np.ndarray:
        """d LML / d log theta (and, after the full form of Observe, d / dX and d / dY) at the last Observe.  It belongs
        to Observe alone: after Absorb, Append, Remove, restore or LaplaceObserve it is refused (GOGP_ESTATE)."""
        g = np.zeros(self._last_len)
        self._check(_lib.lib().gogp_gradient(self._h, _dp(g), g.size))
        return g

    # ---- leave-one-out cross-validation (no reference counterpart: its forecast harness refits per prefix) ----
    def LOO(self):
        """(mu, sigma, logp), n entries each: the prediction of Y[i] -- mean, standard deviation with the noise,
        log density of the observed value -- by the process fitted to the other n - 1 observations, at the
        parameters of the last Absorb / Observe / restore, from the explicit K^-1 (gogp_loo; Rasmussen & Williams
        5.4.2).  ``logp.sum()`` is the LOO-CV score.  Works after Absorb, Observe, Append, Remove and restore and
        leaves the process as it found it.  fp64, unsharded handles only."""
        n = int(_lib.lib().gogp_n(self._h))
        mu, sigma, logp = np.zeros(n), np.zeros(n), np.zeros(n)
        self._check(_lib.lib().gogp_loo(self._h, _dp(mu), _dp(sigma), _dp(logp), None))
        return mu, sigma, logp

    def LOOScore(self) -> float:
        """The LOO-CV score sum(logp) alone, summed on the device in a fixed order (gogp_loo with NULL arrays)."""
        v = ctypes.c_double(0.0)
        self._check(_lib.lib().gogp_loo(self._h, None, None, None, ctypes.byref(v)))
        return v.value

    def LOOGradient(self) -> np.ndarray:
        """d (LOO-CV score) / d log theta, one entry per hyperparameter (gogp_loo_gradient): one extra symmetric
        product for all of them."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_loo_gradient(self._h, _dp(g), g.size))
        return g

    # ---- non-Gaussian likelihoods by the Laplace approximation (no reference counterpart) ----
    def LaplaceObserve(self, x, lik) -> float:
        """The approximate log marginal likelihood of Y under the likelihood ``lik`` -- "bernoulli" (logit link, Y in
        {0, 1}) or "poisson" (log link, counts) -- at x = log theta, by the Laplace approximation around the mode that a
        damped Newton iteration finds (gogp_laplace_observe; Rasmussen & Williams 3.4).  The noise parameter keeps its
        slot: it is the latent nugget.  Drops the regression state (Gradient, Produce, LOO ... need a new Absorb /
        Observe).  Raises ConvergenceError where Newton does not reach the tolerance (the last iterate is stored) and
        ConditionError as Observe does.  fp64, unsharded handles only."""
        xa = _arr(x).reshape(-1)
        if xa.size != self._ns + self._nn:
            raise ValueError("len(x): the Laplace objective takes the hyperparameters only")
        self._push_data()
        self._with_obs = False
        z = ctypes.c_double(0.0)
        rc = _lib.lib().gogp_laplace_observe(self._h, _lik(lik), _dp(xa), xa.size, ctypes.byref(z))
        if rc in (_lib.GOGP_OK, _lib.GOGP_ECOND, _lib.GOGP_ENOCONV):  # stored (and, but for GOGP_OK, reported)
            theta = np.exp(xa)
            self.ThetaSimil = list(theta[:self._ns])
            self.ThetaNoise = list(theta[self._ns:])
        if rc == _lib.GOGP_ENOCONV:
            raise ConvergenceError(_lib.lib().gogp_last_error(self._h).decode(), z.value)
        self._check(rc)
        return z.value

    def LaplaceGradient(self) -> np.ndarray:
        """d LaplaceObserve / d log theta, one entry per hyperparameter, the movement of the mode included
        (gogp_laplace_gradient)."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_laplace_gradient(self._h, _dp(g), g.size))
        return g

    def LaplaceMode(self):
        """(f, a, iterations) of the last LaplaceObserve: the latent values at the mode, a = K^-1 f, and the Newton
        steps taken (gogp_laplace_get_mode)."""
        n = int(_lib.lib().gogp_n(self._h))
        f, a, it = np.zeros(n), np.zeros(n), ctypes.c_int32(0)
        self._check(_lib.lib().gogp_laplace_get_mode(self._h, _dp(f), _dp(a), ctypes.byref(it)))
        return f, a, int(it.value)

    def LaplaceProduce(self, Z, mean: bool = True):
        """(mu, sigma, mean) at the test points Z after a LaplaceObserve: the latent mean and standard deviation (no
        noise, as Produce) and the response-scale prediction -- E[y*] for "poisson", P(y* = 1) for "bernoulli"; None
        with ``mean=False`` (gogp_laplace_produce)."""
        za = _arr(Z).reshape(-1, self.NDim)
        m = za.shape[0]
        mu, sigma = np.zeros(m), np.zeros(m)
        mn = np.zeros(m) if mean else None
        self._check(_lib.lib().gogp_laplace_produce(self._h, _dp(za), m, _dp(mu), _dp(sigma), _dp(mn)))
        return mu, sigma, mn

    # ---- leave-block-out cross-validation (no reference counterpart) ----
    def BlockCV(self, start):
        """(mu, sigma, logp) of leave-block-out cross-validation (gogp_blockcv): the rows are cut into the F
        consecutive blocks [start[f], start[f + 1]) -- start[0] = 0, start[F] = n, 1 .. 128 rows each; ``blocks(n,
        length)`` builds equal ones -- and every block is predicted jointly by the process fitted to all the other
        blocks.  mu, sigma (with the noise): n entries, the held-out prediction of every row; logp: F entries, the joint
        log density of each block's observed values; ``logp.sum()`` is the score.  For time-ordered data this is the
        hold-out that LOO is not; blocks of one row give LOO's values.  Works where LOO works and leaves the process as
        it found it.  Folds that are not contiguous: permute the rows before setting the data."""
        st = _starts(start)
        n = int(_lib.lib().gogp_n(self._h))
        mu, sigma, logp = np.zeros(n), np.zeros(n), np.zeros(st.size - 1)
        self._check(_lib.lib().gogp_blockcv(self._h, _ip(st), st.size - 1, _dp(mu), _dp(sigma), _dp(logp), None))
        return mu, sigma, logp

    def BlockCVScore(self, start) -> float:
        """The block cross-validation score sum(logp) alone, added in block order (gogp_blockcv with NULL arrays)."""
        st = _starts(start)
        v = ctypes.c_double(0.0)
        self._check(_lib.lib().gogp_blockcv(self._h, _ip(st), st.size - 1, None, None, None, ctypes.byref(v)))
        return v.value

    def BlockCVGradient(self, start) -> np.ndarray:
        """d (block cross-validation score) / d log theta, one entry per hyperparameter (gogp_blockcv_gradient)."""
        st = _starts(start)
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_blockcv_gradient(self._h, _ip(st), st.size - 1, _dp(g), g.size))
        return g

    # ---- multi-output: T output columns on one factorisation (no reference counterpart) ----
    def SetOutputs(self, Y) -> None:
        """T output columns observed at the process's inputs, sharing its kernel and hyperparameters (n x T,
        T <= 128; gogp_multi_set_outputs).  Independent of ``Y``, which stays the process's own output vector.  The
        outputs belong to the data on the device: Absorb, the full Observe form, Append, Remove and assigning X / Y
        drop them.  ``None`` clears them.  fp64, unsharded handles only."""
        L = _lib.lib()
        if Y is None:
            self._check(L.gogp_multi_set_outputs(self._h, None, 0, 0))
            self._T = 0
            return
        self._push_data()
        ya = _arr(Y)
        n = len(self._Y)
        if ya.ndim == 1:
            ya = ya.reshape(n, -1) if n else ya.reshape(0, ya.size)
        if ya.ndim != 2:
            raise ValueError("SetOutputs: Y must be n x T")
        ya = np.ascontiguousarray(ya)
        buf = ya if ya.size else np.zeros(1)  # (no observations: a pointer the library may look at)
        self._check(L.gogp_multi_set_outputs(self._h, _dp(buf), ya.shape[0], ya.shape[1]))
        self._T = ya.shape[1]

    def MultiLML(self):
        """(total, per_output): the log marginal likelihood of every output column at the parameters of the last
        Absorb / Observe / restore, and their sum in column order (gogp_multi_lml)."""
        T = getattr(self, "_T", 0)
        total, per = ctypes.c_double(0.0), np.zeros(max(T, 1))
        self._check(_lib.lib().gogp_multi_lml(self._h, ctypes.byref(total), _dp(per)))
        return total.value, per[:T]

    def MultiGradient(self) -> np.ndarray:
        """d (sum of the outputs' LML) / d log theta, one entry per hyperparameter (gogp_multi_gradient): one pass
        over K^-1 for all outputs and all parameters."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_multi_gradient(self._h, _dp(g), g.size))
        return g

    @property
    def MultiAlpha(self) -> np.ndarray:
        """A = K^-1 Y, n x T (gogp_multi_get_alpha)."""
        T = getattr(self, "_T", 0)
        a = np.zeros((int(_lib.lib().gogp_n(self._h)), T))
        buf = a if a.size else np.zeros(1)
        self._check(_lib.lib().gogp_multi_get_alpha(self._h, _dp(buf)))
        return a

    def MultiProduce(self, x):
        """(mu, sigma): the predictive means of every output at the test points, m x T, and the standard deviation
        they share, m entries, as Produce returns it (gogp_multi_produce)."""
        z = _arr(x).reshape(-1, self.NDim)
        m, T = len(z), getattr(self, "_T", 0)
        mu, sigma = np.zeros((m, T)), np.zeros(m)
        buf = mu if mu.size else np.zeros(1)
        self._check(_lib.lib().gogp_multi_produce(self._h, _dp(z) if m else None, m, _dp(buf), _dp(sigma) if m else None))
        return mu, sigma

    # ---- explicit basis functions: a marginalised linear mean (no reference counterpart) ----
    def SetBasis(self, H) -> None:
        """The basis functions of a mean h(x)^T beta at the process's inputs (n x p, p <= 64, p < n; gogp_basis_set;
        gogp_amd.basis builds such matrices); beta is integrated out under a flat prior (Rasmussen & Williams section
        2.7).  The basis belongs to the data on the device: the full Observe form, Append, Remove and assigning X / Y
        drop it.  ``None`` clears it.  fp64, unsharded handles only.  Option "basis_symm" (-1 | 0 | 1) chooses how
        K^-1 H is formed: from the explicit K^-1 where a gradient has left it on the device (the default), or always
        from the factor (0) / from K^-1 (1)."""
        L = _lib.lib()
        if H is None:
            self._check(L.gogp_basis_set(self._h, None, 0, 0))
            self._p = 0
            return
        self._push_data()
        ha = _arr(H)
        n = len(self._Y)
        if ha.ndim == 1:
            ha = ha.reshape(n, -1) if n else ha.reshape(0, ha.size)
        if ha.ndim != 2:
            raise ValueError("SetBasis: H must be n x p")
        ha = np.ascontiguousarray(ha)
        buf = ha if ha.size else np.zeros(1)
        self._check(L.gogp_basis_set(self._h, _dp(buf), ha.shape[0], ha.shape[1]))
        self._p = ha.shape[1]

    def BasisLML(self) -> float:
        """The log marginal likelihood with beta integrated out (R&W eq. 2.45 in the flat-prior limit) at the
        parameters of the last Absorb / Observe / restore (gogp_basis_lml)."""
        v = ctypes.c_double(0.0)
        self._check(_lib.lib().gogp_basis_lml(self._h, ctypes.byref(v)))
        return v.value

    def BasisGradient(self) -> np.ndarray:
        """d BasisLML / d log theta, one entry per hyperparameter (gogp_basis_gradient)."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_basis_gradient(self._h, _dp(g), g.size))
        return g

    def BasisBeta(self):
        """(beta, cov): the estimate of the mean's coefficients, p entries, and its covariance (H^T K^-1 H)^-1, p x p
        (gogp_basis_get_beta)."""
        p = max(getattr(self, "_p", 0), 1)
        beta, cov = np.zeros(p), np.zeros((p, p))
        self._check(_lib.lib().gogp_basis_get_beta(self._h, _dp(beta), _dp(cov)))
        return beta, cov

    @property
    def BasisAlpha(self) -> np.ndarray:
        """alpha~ = K^-1 (y - H beta), n entries (gogp_basis_get_alpha)."""
        a = np.zeros(max(int(_lib.lib().gogp_n(self._h)), 1))
        self._check(_lib.lib().gogp_basis_get_alpha(self._h, _dp(a)))
        return a

    def BasisProduce(self, x, Hz):
        """(mu, sigma) at the test points ``x`` whose basis functions are the rows of ``Hz`` (m x p): Produce's mean plus
        the mean's contribution, and the standard deviation widened by the uncertainty of beta (gogp_basis_produce)."""
        z = _arr(x).reshape(-1, self.NDim)
        m = len(z)
        hz = _arr(Hz)
        # (an m x 0 array: no basis is set, and the library says so as BasisLML does, with GOGP_ESTATE)
        hz = np.ascontiguousarray(hz.reshape(m, -1)) if m and hz.size else np.zeros((m, 0))
        if m and hz.shape[1] != getattr(self, "_p", 0):
            raise ValueError("BasisProduce: Hz must be m x p")
        mu, sigma = np.zeros(m), np.zeros(m)
        buf = hz if hz.size else np.zeros(1)  # (no basis: a pointer the library may look at)
        self._check(_lib.lib().gogp_basis_produce(self._h, _dp(z) if m else None, _dp(buf) if m else None, m,
                                                  _dp(mu) if m else None, _dp(sigma) if m else None))
        return mu, sigma

    # ---- sparse: the collapsed bound on M inducing points (no reference counterpart) ----
    def SetSparse(self, X, Y, U) -> None:
        """Data of the inducing-point approximation (gogp_sparse_set_data): N observations X (N x NDim), Y and
        M <= 4096 inducing points U (M x NDim), kept on the device beside the process's own X / Y, which they do not
        touch.  ``U = None`` clears them.  fp64, unsharded handles without event discounts only."""
        L = _lib.lib()
        if U is None:
            self._check(L.gogp_sparse_set_data(self._h, None, None, 0, None, 0))
            self._sparse_m = self._sparse_t = 0
            return
        u = np.ascontiguousarray(_arr(U).reshape(-1, self.NDim))
        x = np.ascontiguousarray(_arr(X).reshape(-1, self.NDim))
        y = np.ascontiguousarray(_arr(Y).reshape(-1))
        if len(x) != len(y):
            raise ValueError("SetSparse: len(X) != len(Y)")
        n = len(y)
        self._check(L.gogp_sparse_set_data(self._h, _dp(x) if n else None, _dp(y) if n else None, n,
                                           _dp(u if len(u) else np.zeros(1)), len(u)))
        self._sparse_m = len(u)
        self._sparse_t = 0  # (the library drops the outputs of SetSparseOutputs with the data they rode on)

    def SetInducing(self, U) -> None:
        """Replace the inducing points of SetSparse by U (M x NDim, the same M) and nothing else
        (gogp_sparse_set_inducing): X, Y and every device buffer stay.  SparseObserve has to follow before a gradient
        or a forecast."""
        u = np.ascontiguousarray(_arr(U).reshape(-1, self.NDim))
        self._check(_lib.lib().gogp_sparse_set_inducing(self._h, _dp(u if len(u) else np.zeros(1)), len(u)))

    def SelectInducing(self, x, M: int, X=None, tol=None):
        """(idx, U, pivots, trace): greedy conditional-variance selection of at most M inducing points among the rows of
        X at x = log theta (gogp_sparse_select_inducing) -- a partial Cholesky factorisation of k(X, X) with diagonal
        pivoting; the noise does not enter.  ``X = None`` selects among the rows of the sparse data already on the device
        (gogp_sparse_select_inducing_resident).  The selection stops once no residual variance exceeds ``tol`` (None: the
        jitter 10^"sparse_jitter_log10"), so the arrays are cut to the m <= M points taken: idx their rows in pick order,
        U = X[idx], pivots the residual variances at the picks, trace = t0 - tr Qff for these inducing points.  Nothing of
        the process's state changes."""
        xa = np.ascontiguousarray(_arr(x).reshape(-1))
        M = int(M)
        cap = max(M, 1)
        idx, piv, U = np.zeros(cap, dtype=np.int64), np.zeros(cap), np.zeros((cap, self.NDim))
        m, tr = ctypes.c_int64(0), ctypes.c_double(0.0)
        t = -1.0 if tol is None else float(tol)
        L = _lib.lib()
        if X is None:
            rc = L.gogp_sparse_select_inducing_resident(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size, M, t,
                                                        _ip(idx), _dp(piv), _dp(U), ctypes.byref(m), ctypes.byref(tr))
        else:
            xs = np.ascontiguousarray(_arr(X).reshape(-1, self.NDim))
            rc = L.gogp_sparse_select_inducing(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size,
                                               _dp(xs) if len(xs) else None, len(xs), M, t, _ip(idx), _dp(piv), _dp(U),
                                               ctypes.byref(m), ctypes.byref(tr))
        self._check(rc)
        k = m.value
        return idx[:k].copy(), U[:k].copy(), piv[:k].copy(), tr.value

    def SetSparseGreedy(self, X, Y, M: int, x, tol=None) -> np.ndarray:
        """SelectInducing(x, M, X, tol) followed by SetSparse(X, Y, U) with the points it took; returns their rows idx
        (m <= M of them: the sparse data then has m inducing points)."""
        idx, U, _, _ = self.SelectInducing(x, M, X=X, tol=tol)
        self.SetSparse(X, Y, U)
        return idx

    # ---- the iterative exact GP: matrix-free preconditioned conjugate gradients (gogp_cg_*) ----
    def SetCG(self, X, Y, v=None) -> None:
        """The data of the iterative calls, a set of their own that stays on the device (gogp_cg_set_data): X (N x
        NDim), Y (N) and, optionally, per-observation noise variances v (N, finite and >= 0).  ``SetCG(None, None)``
        clears them.  Nothing else of the process changes."""
        if X is None and Y is None and v is None:
            self._cg_n = 0
            self._check(_lib.lib().gogp_cg_set_data(self._h, None, None, None, 0))
            return
        xs = np.ascontiguousarray(_arr(X).reshape(-1, self.NDim))
        ys = np.ascontiguousarray(_arr(Y).reshape(-1))
        if len(xs) != len(ys):
            raise ValueError("SetCG: len(X) != len(Y)")
        va = None
        if v is not None:
            va = np.ascontiguousarray(_arr(v).reshape(-1))
            if va.size != len(ys):
                raise ValueError("SetCG: one variance per observation")
        self._check(_lib.lib().gogp_cg_set_data(self._h, _dp(xs) if len(xs) else None, _dp(ys) if len(ys) else None,
                                                _dp(va), len(ys)))
        self._cg_n = len(ys)

    @staticmethod
    def _cg_cols(cols, k):
        return {"iterations": np.array([cols[i].iterations for i in range(k)], dtype=np.int64),
                "converged": np.array([bool(cols[i].converged) for i in range(k)]),
                "rel_residual": np.array([cols[i].rel_residual for i in range(k)]),
                "rel_residual_recurrence": np.array([cols[i].rel_residual_recurrence for i in range(k)])}

    def _cg_info(self) -> dict:
        info = _lib.CCgInfo()
        self._check(_lib.lib().gogp_cg_last_info(self._h, ctypes.byref(info)))
        return {"rank_used": int(info.rank_used), "products": int(info.products), "blocks": int(info.blocks),
                "yt_alpha": float(info.yt_alpha)}

    def _cg_finish(self, rc: int, result):
        """GOGP_ENOCONV raises ConvergenceError carrying the results that were written; other errors as usual."""
        if rc == _lib.GOGP_ENOCONV:
            e = ConvergenceError(_lib.lib().gogp_last_error(self._h).decode())
            e.result = result
            raise e
        self._check(rc)
        return result

    def CGSolve(self, x, rank: int = 64, tol: float = 1e-8, max_iter: int = 1000, piv_tol=None) -> dict:
        """Solve K^ alpha = Y at x = log theta by preconditioned conjugate gradients, K^ = k(X, X) + sigma^2 I + diag(v)
        never stored (gogp_cg_solve).  The preconditioner is a pivoted-Cholesky factor of k(X, X) of at most ``rank``
        columns (0: Jacobi) that stops once no residual variance exceeds ``piv_tol`` (None: the sparse calls' jitter).
        Returns the info fields (rank_used, products, blocks, yt_alpha) and the column's iterations, converged,
        rel_residual (true, from one more product) and rel_residual_recurrence.  alpha, theta and the preconditioner
        stay for CGAlpha, CGSolveColumns and CGProduce.  Not converged within max_iter: ConvergenceError whose
        ``result`` is this dict; alpha is stored all the same."""
        xa = np.ascontiguousarray(_arr(x).reshape(-1))
        info, col = _lib.CCgInfo(), (_lib.CCgCol * 1)()
        rc = _lib.lib().gogp_cg_solve(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size, int(rank),
                                      -1.0 if piv_tol is None else float(piv_tol), float(tol), int(max_iter),
                                      ctypes.byref(info), col)
        out = {"rank_used": int(info.rank_used), "products": int(info.products), "blocks": int(info.blocks),
               "yt_alpha": float(info.yt_alpha)}
        out.update({k: v[0] for k, v in self._cg_cols(col, 1).items()})
        self.cg_info = out
        return self._cg_finish(rc, out)

    def CGAlpha(self) -> np.ndarray:
        """alpha of the last CGSolve (gogp_cg_get_alpha)."""
        a = np.zeros(max(int(getattr(self, "_cg_n", 0)), 1))
        self._check(_lib.lib().gogp_cg_get_alpha(self._h, _dp(a), int(getattr(self, "_cg_n", 0))))
        return a[:int(getattr(self, "_cg_n", 0))]

    def CGSolveColumns(self, B, tol: float = 1e-8, max_iter: int = 1000):
        """(S, cols): K^ S[t] = B[t] for the T rows of B (T x N), in lock-step blocks of 64, with the parameters and
        preconditioner of the last CGSolve (gogp_cg_solve_columns).  cols: the per-column arrays of CGSolve.  A column
        has the same bits alone as inside a block."""
        n = int(getattr(self, "_cg_n", 0))
        b = np.ascontiguousarray(_arr(B).reshape(-1, n) if n else _arr(B).reshape(0, 0))
        T = len(b)
        S = np.zeros((T, n))
        cols = (_lib.CCgCol * max(T, 1))()
        rc = _lib.lib().gogp_cg_solve_columns(self._h, _dp(b) if T else None, T, float(tol), int(max_iter),
                                              _dp(S) if T else None, cols)
        self.cg_info = self._cg_info()
        return self._cg_finish(rc, (S, self._cg_cols(cols, T)))

    def CGProduce(self, z, sigma: bool = True, tol: float = 1e-8, max_iter: int = 1000):
        """(mu, sigma) of the exact posterior at the test points z (m x NDim), latent and unclamped as Produce
        (gogp_cg_produce): the mean is one rectangular matrix-free product with alpha; the deviations take one solve
        per test point, 64 at a time.  ``sigma=False`` returns (mu, None) without any solve.  ``cg_info`` and
        ``cg_cols`` keep the counters and the per-column results of the call."""
        zs = np.ascontiguousarray(_arr(z).reshape(-1, self.NDim))
        m = len(zs)
        mu = np.zeros(m)
        sg = np.zeros(m) if sigma else None
        cols = (_lib.CCgCol * max(m, 1))()
        rc = _lib.lib().gogp_cg_produce(self._h, _dp(zs) if m else None, m, _dp(mu) if m else None,
                                        _dp(sg) if (sigma and m) else None, float(tol), int(max_iter), cols)
        self.cg_info = self._cg_info()
        self.cg_cols = self._cg_cols(cols, m)
        return self._cg_finish(rc, (mu, sg))

    _cg_normals_cache: dict = {}

    @classmethod
    def _cg_normals(cls, seed: int, n: int, rank: int, probes: int) -> np.ndarray:
        """The probes' standard normals, probes x (n + rank), drawn once per (seed, n, rank, probes) and read only: the
        same probes serve every theta (common random numbers)."""
        key = (int(seed), int(n), int(rank), int(probes))
        xi = cls._cg_normals_cache.get(key)
        if xi is None:
            if len(cls._cg_normals_cache) >= 4:
                cls._cg_normals_cache.clear()
            xi = np.random.default_rng(key[0]).standard_normal((key[3], key[1] + key[2]))
            xi.setflags(write=False)
            cls._cg_normals_cache[key] = xi
        return xi

    def CGObserve(self, x, probes: int = 16, seed: int = 0, rank: int = 64, tol: float = 1e-8, max_iter: int = 1000,
                  piv_tol=None, xi=None) -> float:
        """The log marginal likelihood of the CG data at x = log theta by stochastic Lanczos quadrature (CGSolve, then
        gogp_cg_lml_gradient): ``probes`` probe vectors z = D^1/2 (Ls xi1 + xi2) ~ N(0, P), one preconditioned solve
        each, the log-determinant from the solves' own CG coefficients and the gradient's trace term from the same
        solves.  The normals come from numpy.random.default_rng(seed), drawn once per (seed, N, rank, probes), or from
        ``xi`` (probes x (N + rank); the first N + rank_used columns of a row are used: [xi2 | xi1]).  The gradient is
        kept for CGGradient; ``cg_lml_info`` holds lml, yt_alpha, logdet, logdet_precond, logdet_stderr, probes, blocks,
        products, lanczos_max, quad (per probe) and the per-column arrays of CGSolve.  Not converged within max_iter:
        ConvergenceError whose ``result`` is the estimate from the columns as they stand."""
        n = int(getattr(self, "_cg_n", 0))
        if int(probes) < 1:
            raise ValueError("CGObserve: probes >= 1")
        if int(rank) < 0:
            raise ValueError("CGObserve: rank >= 0")
        if xi is None:
            xs = self._cg_normals(seed, n, int(rank), int(probes))
        else:
            xs = np.ascontiguousarray(_arr(xi))
            if xs.ndim != 2 or xs.shape[0] != int(probes) or xs.shape[1] < n + int(rank):
                raise ValueError("CGObserve: xi is probes x (N + rank)")
        try:
            self.CGSolve(x, rank=rank, tol=tol, max_iter=max_iter, piv_tol=piv_tol)
            noconv = None
        except ConvergenceError as e:
            noconv = e
        t, p = xs.shape[0], self._ns + self._nn
        g, quad = np.zeros(max(p, 1)), np.zeros(t)
        info, cols = _lib.CCgLmlInfo(), (_lib.CCgCol * t)()
        rc = _lib.lib().gogp_cg_lml_gradient(self._h, _dp(xs), t, xs.shape[1], float(tol), int(max_iter), _dp(g), p,
                                             _dp(quad), ctypes.byref(info), cols)
        out = {k: float(getattr(info, k)) for k in ("lml", "yt_alpha", "logdet", "logdet_precond", "logdet_stderr")}
        out.update({k: int(getattr(info, k)) for k in ("probes", "blocks", "products", "lanczos_max")})
        out["quad"] = quad
        out.update(self._cg_cols(cols, t))
        self.cg_lml_info = out
        self._cg_grad = g[:p] if rc in (_lib.GOGP_OK, _lib.GOGP_ENOCONV) else None
        if rc == _lib.GOGP_OK and noconv is not None:
            noconv.result = out["lml"]
            raise noconv
        return self._cg_finish(rc, out["lml"])

    def CGGradient(self) -> np.ndarray:
        """d LML / d log theta of the last CGObserve (the estimate of gogp_cg_lml_gradient)."""
        g = getattr(self, "_cg_grad", None)
        if g is None:
            raise GogpError(_lib.GOGP_ESTATE, "CGGradient before CGObserve")
        return g.copy()

    # ---- Vecchia's approximation: nearest-neighbour conditionals (gogp_vecchia_*) ----
    @staticmethod
    def _vecchia_table(neighbours, rows: int, what: str) -> np.ndarray:
        t = np.ascontiguousarray(np.asarray(neighbours, dtype=np.int32))
        if t.ndim != 2 or t.shape[0] != rows:
            raise ValueError("%s: the table has one row per target (%d x m int32)" % (what, rows))
        return t

    def SetVecchia(self, x, y, neighbours, v=None) -> None:
        """The data of the Vecchia calls, a set of their own that stays on the device (gogp_vecchia_set_data): x (N x
        NDim), y (N), the table ``neighbours`` (N x m int32, m <= 63: row i holds distinct indices below i, then -1
        padding; gogp_amd.vecchia.previous / nearest build one) and, optionally, per-observation noise variances v.
        ``SetVecchia(None, None, None)`` clears them.  Nothing else of the process changes."""
        if x is None and y is None and neighbours is None and v is None:
            self._vc_n, self._vc_m = 0, 0
            self._check(_lib.lib().gogp_vecchia_set_data(self._h, None, None, None, 0, None, 0))
            return
        xs = np.ascontiguousarray(_arr(x).reshape(-1, self.NDim))
        ys = np.ascontiguousarray(_arr(y).reshape(-1))
        if len(xs) != len(ys):
            raise ValueError("SetVecchia: len(x) != len(y)")
        t = self._vecchia_table(neighbours, len(ys), "SetVecchia")
        va = None
        if v is not None:
            va = np.ascontiguousarray(_arr(v).reshape(-1))
            if va.size != len(ys):
                raise ValueError("SetVecchia: one variance per observation")
        self._vc_terms = None
        self._check(_lib.lib().gogp_vecchia_set_data(self._h, _dp(xs) if len(xs) else None, _dp(ys) if len(ys) else None,
                                                     _dp(va), len(ys), _i32p(t) if t.size else None, t.shape[1]))
        self._vc_n, self._vc_m = len(ys), t.shape[1]

    def VecchiaObserve(self, theta) -> float:
        """Vecchia's approximation of the LML at theta = log of the hyperparameters (gogp_vecchia_observe): the sum of the
        N conditionals' log densities.  A valid joint density, not a bound; exact when every row conditions on all earlier
        ones.  The terms are kept for VecchiaTerms()."""
        xa = np.ascontiguousarray(_arr(theta).reshape(-1))
        n = getattr(self, "_vc_n", 0)
        terms = np.zeros((max(n, 1), 3))
        val = ctypes.c_double(0.0)
        self._vc_terms = None
        rc = _lib.lib().gogp_vecchia_observe(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size, ctypes.byref(val),
                                             _dp(terms))
        if rc in (_lib.GOGP_OK, _lib.GOGP_ENOTPD):
            self._vc_terms = terms[:n]
        self._check(rc)
        return val.value

    def VecchiaTerms(self):
        """(mu, s, logp) of the last VecchiaObserve, N each: the one-step-ahead forecast of y_i from its conditioning rows
        (s includes the noise) and its log density.  After a FactorizeError the failing rows hold NaN."""
        t = getattr(self, "_vc_terms", None)
        if t is None:
            raise GogpError(_lib.GOGP_ESTATE, "VecchiaTerms before VecchiaObserve")
        return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()

    def VecchiaGradient(self) -> np.ndarray:
        """d value / d log theta at the parameters of the last VecchiaObserve (gogp_vecchia_gradient): the exact derivative
        of VecchiaObserve's value, the noise parameter's component included."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_vecchia_gradient(self._h, _dp(g if g.size else np.zeros(1)), g.size))
        return g

    def VecchiaProduce(self, z, neighbours, sigma: bool = True):
        """(mu, sigma) at the test points z, each conditioned on the rows of the Vecchia data its row of ``neighbours``
        (len(z) x m, the m of SetVecchia; gogp_amd.vecchia.nearest_to builds one) names, at the parameters of the last
        VecchiaObserve; latent and unclamped as Produce (gogp_vecchia_produce).  ``sigma=False`` returns (mu, None)."""
        zz = np.ascontiguousarray(_arr(z).reshape(-1, self.NDim))
        mz = len(zz)
        t = self._vecchia_table(neighbours, mz, "VecchiaProduce")
        if t.shape[1] != getattr(self, "_vc_m", 0):  # the library reads mz x m entries, the m of SetVecchia
            raise ValueError("VecchiaProduce: the table has %d columns, SetVecchia's has %d" % (t.shape[1], getattr(self, "_vc_m", 0)))
        mu = np.zeros(mz)
        sg = np.zeros(mz) if sigma else None
        self._check(_lib.lib().gogp_vecchia_produce(self._h, _dp(zz) if mz else None, mz, _i32p(t) if t.size else None,
                                                    _dp(mu) if mz else None, _dp(sg) if mz and sigma else None))
        return mu, sg

    # ---- ... with the table built on the device (vecchia_knn.hip): the search of vecchia.nearest / nearest_to ----
    def _vecchia_lengths(self, lengths, what: str):
        """``lengths`` as the host helpers take it -- a scalar or one value per dimension -- as NDim doubles; None stays."""
        if lengths is None:
            return None
        la = np.asarray(lengths, dtype=np.float64)
        if la.ndim > 1 or (la.ndim == 1 and la.size != self.NDim):
            raise ValueError("%s: lengths is a scalar or one value per dimension (%d)" % (what, self.NDim))
        la = np.ascontiguousarray(np.broadcast_to(la, (self.NDim,)))
        if not np.all(np.isfinite(la) & (la > 0.0)):
            raise ValueError("%s: lengths must be positive and finite" % what)
        return la

    @staticmethod
    def _vecchia_m(m, what: str) -> int:
        m = int(m)
        if not 0 <= m <= 63:
            raise ValueError("%s: m: 0 .. 63 conditioning rows" % what)
        return m

    def _vecchia_rows(self, a, what: str) -> np.ndarray:
        a = _arr(a)
        if a.ndim == 2 and a.shape[1] != self.NDim:
            raise ValueError("%s: rows of %d values, not %d" % (what, self.NDim, a.shape[1]))
        if a.size % self.NDim:
            raise ValueError("%s: rows of %d values" % (what, self.NDim))
        return np.ascontiguousarray(a.reshape(-1, self.NDim))

    def VecchiaNeighbours(self, x, m: int, lengths=None, z=None) -> np.ndarray:
        """The table of vecchia.nearest(x, m, lengths) -- or, with test points ``z``, of vecchia.nearest_to(x, z, m,
        lengths) -- found on the device, integer for integer (gogp_vecchia_neighbours).  One-shot: nothing of the process
        changes."""
        what = "VecchiaNeighbours"
        m = self._vecchia_m(m, what)
        xs = self._vecchia_rows(x, what + ": x")
        la = self._vecchia_lengths(lengths, what)
        zz = None if z is None else self._vecchia_rows(z, what + ": z")
        rows = len(xs) if zz is None else len(zz)
        t = np.full((rows, m), -1, dtype=np.int32)
        if len(xs) == 0 or rows == 0 or m == 0:
            return t
        self._check(_lib.lib().gogp_vecchia_neighbours(self._h, _dp(xs), len(xs), None if zz is None else _dp(zz),
                                                       0 if zz is None else len(zz), _dp(la), m, _i32p(t)))
        return t

    def SetVecchiaNearest(self, x, y, m: int, lengths=None, v=None) -> None:
        """SetVecchia(x, y, vecchia.nearest(x, m, lengths), v) with the table built on the device from the uploaded x, where
        it stays (gogp_vecchia_set_data_nearest).  VecchiaNeighbourTable() returns it, VecchiaReneighbour rebuilds it."""
        what = "SetVecchiaNearest"
        m = self._vecchia_m(m, what)
        xs = self._vecchia_rows(x, what + ": x")
        ys = np.ascontiguousarray(_arr(y).reshape(-1))
        if len(xs) != len(ys):
            raise ValueError("SetVecchiaNearest: len(x) != len(y)")
        la = self._vecchia_lengths(lengths, what)
        va = None
        if v is not None:
            va = np.ascontiguousarray(_arr(v).reshape(-1))
            if va.size != len(ys):
                raise ValueError("SetVecchiaNearest: one variance per observation")
        self._vc_terms = None
        self._check(_lib.lib().gogp_vecchia_set_data_nearest(self._h, _dp(xs) if len(xs) else None,
                                                             _dp(ys) if len(ys) else None, _dp(va), len(ys), _dp(la), m))
        self._vc_n, self._vc_m = len(ys), m

    def VecchiaReneighbour(self, lengths) -> None:
        """Rebuild the resident table from the resident x under new length scales, same m (gogp_vecchia_reneighbour); also
        on data that SetVecchia brought with a table, which it replaces.  The last VecchiaObserve is dropped."""
        la = self._vecchia_lengths(lengths, "VecchiaReneighbour")
        self._vc_terms = None
        self._check(_lib.lib().gogp_vecchia_reneighbour(self._h, _dp(la)))

    def VecchiaNeighbourTable(self) -> np.ndarray:
        """The resident table, N x m int32 (gogp_vecchia_get_neighbours)."""
        t = np.full((getattr(self, "_vc_n", 0), getattr(self, "_vc_m", 0)), -1, dtype=np.int32)
        self._check(_lib.lib().gogp_vecchia_get_neighbours(self._h, _i32p(t) if t.size else None))
        return t

    def VecchiaProduceNearest(self, z, lengths=None, sigma: bool = True, table: bool = False):
        """VecchiaProduce(z, vecchia.nearest_to(x, z, m, lengths)) with the table found on the device
        (gogp_vecchia_produce_nearest); ``lengths=None``: those the resident table was built with (refused with GOGP_ESTATE
        where the caller brought the table: SetVecchia).  Returns (mu, sigma), or
        (mu, sigma, table) with ``table=True``."""
        what = "VecchiaProduceNearest"
        zz = self._vecchia_rows(z, what + ": z")
        la = self._vecchia_lengths(lengths, what)
        mz, m = len(zz), getattr(self, "_vc_m", 0)
        mu = np.zeros(mz)
        sg = np.zeros(mz) if sigma else None
        t = np.full((mz, m), -1, dtype=np.int32) if table else None
        self._check(_lib.lib().gogp_vecchia_produce_nearest(
            self._h, _dp(zz) if mz else None, mz, _dp(la), _dp(mu) if mz else None, _dp(sg) if mz and sigma else None,
            _i32p(t) if table and t.size else None))
        return (mu, sg, t) if table else (mu, sg)

    def SparseObserve(self, x) -> float:
        """The collapsed variational bound of Titsias (2009) at x = log theta (gogp_sparse_observe): a lower bound of
        the LML of the sparse data that costs O(N M^2).  SparseObserve and SparseMultiObserve share one workspace: the
        last one of either flavour owns it, and the other flavour's gradient and forecast are refused (GOGP_ESTATE)
        until it observes again."""
        xa = np.ascontiguousarray(_arr(x).reshape(-1))
        v = ctypes.c_double(0.0)
        self._check(_lib.lib().gogp_sparse_observe(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size, ctypes.byref(v)))
        return v.value

    def SparseGradient(self) -> np.ndarray:
        """d bound / d log theta at the parameters of the last SparseObserve (gogp_sparse_gradient)."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_sparse_gradient(self._h, _dp(g if g.size else np.zeros(1)), g.size))
        return g

    def SparseGradientInducing(self):
        """(grad, dU): SparseGradient() and, from the same pass over the data, the derivative of the bound in the
        inducing points, M x NDim (gogp_sparse_gradient_inducing).  Where Kuu is ill-conditioned (thousands of
        inducing points at the default jitter of 1e-8) dU loses its digits before grad does: set option
        "sparse_jitter_log10" to -6 or more to learn that many (include/gogp_hip.h has the measurements)."""
        g = np.zeros(self._ns + self._nn)
        if self._sparse_m < 1:  # (the library writes M x NDim doubles: never into a buffer sized without M)
            raise GogpError(_lib.GOGP_ESTATE, "SparseGradientInducing before SetSparse")
        du = np.zeros((self._sparse_m, self.NDim))
        self._check(_lib.lib().gogp_sparse_gradient_inducing(self._h, _dp(g if g.size else np.zeros(1)), g.size, _dp(du)))
        return g, du

    def SparseProduce(self, x):
        """(mu, sigma) of the sparse approximation at the test points, latent and unclamped as Produce
        (gogp_sparse_produce)."""
        z = np.ascontiguousarray(_arr(x).reshape(-1, self.NDim))
        m = len(z)
        mu, sigma = np.zeros(m), np.zeros(m)
        self._check(_lib.lib().gogp_sparse_produce(self._h, _dp(z) if m else None, m, _dp(mu) if m else None,
                                                   _dp(sigma) if m else None))
        return mu, sigma

    # ---- sparse multi-output: T output columns on one pass over the sparse data ----
    def SetSparseOutputs(self, Y) -> None:
        """The T <= 128 output columns observed at the inputs of SetSparse (gogp_sparse_multi_set_outputs): Y is N x T
        (a vector is one column), copied to the device as given.  ``Y = None`` clears them; SetSparse drops them,
        SetInducing keeps them."""
        L = _lib.lib()
        if Y is None:
            self._check(L.gogp_sparse_multi_set_outputs(self._h, None, 0, 0))
            self._sparse_t = 0
            return
        ya = _arr(Y)
        if ya.ndim == 1:
            ya = ya.reshape(-1, 1)
        if ya.ndim != 2:
            raise ValueError("SetSparseOutputs: Y must be N x T")
        ya = np.ascontiguousarray(ya)
        buf = ya if ya.size else np.zeros(1)  # (no observations: a pointer the library may look at)
        self._check(L.gogp_sparse_multi_set_outputs(self._h, _dp(buf), ya.shape[0], ya.shape[1]))
        self._sparse_t = ya.shape[1]

    def SparseMultiObserve(self, x):
        """(total, bounds): the collapsed bound of every output column at x = log theta and their sum in column order
        (gogp_sparse_multi_observe): one pass over the data for all of them.  It takes the workspace it shares with
        SparseObserve: SparseGradient and SparseProduce are refused (GOGP_ESTATE) until the next SparseObserve."""
        xa = np.ascontiguousarray(_arr(x).reshape(-1))
        T = getattr(self, "_sparse_t", 0)
        total, per = ctypes.c_double(0.0), np.zeros(max(T, 1))
        self._check(_lib.lib().gogp_sparse_multi_observe(self._h, _dp(xa if xa.size else np.zeros(1)), xa.size,
                                                         ctypes.byref(total), _dp(per)))
        return total.value, per[:T]

    def SparseMultiGradient(self) -> np.ndarray:
        """d total / d log theta at the parameters of the last SparseMultiObserve (gogp_sparse_multi_gradient)."""
        g = np.zeros(self._ns + self._nn)
        self._check(_lib.lib().gogp_sparse_multi_gradient(self._h, _dp(g if g.size else np.zeros(1)), g.size))
        return g

    def SparseMultiGradientInducing(self):
        """(grad, dU): SparseMultiGradient() and, from the same pass over the data, the derivative of the total in the
        inducing points, M x NDim (gogp_sparse_multi_gradient_inducing); the caveats of SparseGradientInducing."""
        g = np.zeros(self._ns + self._nn)
        if getattr(self, "_sparse_m", 0) < 1:  # (the library writes M x NDim doubles: never into a buffer sized without M)
            raise GogpError(_lib.GOGP_ESTATE, "SparseMultiGradientInducing before SetSparse")
        du = np.zeros((self._sparse_m, self.NDim))
        self._check(_lib.lib().gogp_sparse_multi_gradient_inducing(self._h, _dp(g if g.size else np.zeros(1)), g.size,
                                                                   _dp(du)))
        return g, du

    def SparseMultiProduce(self, x):
        """(mu, sigma): the means of every output at the test points, m x T, and the standard deviation they share, m
        entries, latent and unclamped as SparseProduce (gogp_sparse_multi_produce)."""
        z = np.ascontiguousarray(_arr(x).reshape(-1, self.NDim))
        m, T = len(z), getattr(self, "_sparse_t", 0)
        mu, sigma = np.zeros((m, T)), np.zeros(m)
        buf = mu if mu.size else np.zeros(1)
        self._check(_lib.lib().gogp_sparse_multi_produce(self._h, _dp(z) if m else None, m, _dp(buf) if m else None,
                                                         _dp(sigma) if m else None))
        return mu, sigma

    # ---- cached computations: gp.GP.L, gp.GP.Alpha (gp/gp.go:34-37) ----------------------
    @property
    def Alpha(self) -> np.ndarray:
        n = int(_lib.lib().gogp_n(self._h))
        a = np.zeros(n)
        if n:
            self._check(_lib.lib().gogp_get_alpha(self._h, _dp(a)))
        return a

    @property
    def L(self) -> np.ndarray:
        """Lower Cholesky factor (gonum's mat.Cholesky holds U = L^T)."""
        n = int(_lib.lib().gogp_n(self._h))
        out = np.zeros((n, n))
        if n:
            self._check(_lib.lib().gogp_get_factor(self._h, _dp(out)))
        return out

    def L_rows(self, rows) -> np.ndarray:
        """Selected rows of L (len(rows) x n), for checks at sizes where the whole factor
        is not wanted on the host."""
        n = int(_lib.lib().gogp_n(self._h))
        idx = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        out = np.zeros((idx.size, n))
        if n and idx.size:
            self._check(_lib.lib().gogp_get_factor_rows(
                self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), idx.size, _dp(out)))
        return out

    def L_diag(self) -> np.ndarray:
        n = int(_lib.lib().gogp_n(self._h))
        d = np.zeros(n)
        if n:
            self._check(_lib.lib().gogp_get_factor_diag(self._h, _dp(d)))
        return d

    def restore(self, L, Alpha) -> None:
        """Produce on stored results (gp/gp.go:255-257): re-install ThetaSimil,
        ThetaNoise, X, L, Alpha without refactorising."""
        self._push_data()
        ts = _arr(self.ThetaSimil)
        tn = _arr(self.ThetaNoise) if self._nn else np.zeros(1)
        Lm, al = _arr(L), _arr(Alpha)
        self._check(_lib.lib().gogp_set_factor(self._h, _dp(ts), _dp(tn), _dp(Lm), _dp(al)))

    # ---- measurement hooks ----------------------------------------------------------------
    def graph_info(self):
        """(nodes of the candidates' launch graph in use, whether the runtime refused an explicitly built graph)."""
        nodes, refused = ctypes.c_int64(0), ctypes.c_int(0)
        self._check(_lib.lib().gogp_graph_info(self._h, ctypes.byref(nodes), ctypes.byref(refused)))
        return int(nodes.value), bool(refused.value)

    def set_option(self, name: str, value: int):
        """gogp_set_option; include/gogp_hip.h lists the options.  "gradient_precision" = 32 (K^-1 in float for Gradient
        alone) is refused while noise variances are set (GOGP_EARG); while it holds, SetNoiseVariances and the calls that
        read an fp64 K^-1 -- LOO, BlockCV, NoiseVariancesGradient, the Multi* and Basis* calls -- and LaplaceObserve,
        LaplaceGradient and LaplaceProduce are refused with GOGP_EARG (LaplaceMode still copies out a stored mode); LML,
        Alpha, Produce and the candidates are unchanged.  Setting it (to either value)
        drops a stored K^-1 and gradient, nothing else."""
        self._check(_lib.lib().gogp_set_option(self._h, name.encode(), int(value)))

    def profile_enable(self, on: bool = True):
        self._check(_lib.lib().gogp_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """(sum of launch durations ms, launches, launched flops, union busy ms)"""
        ms, nl, fl, bz = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(_lib.lib().gogp_profile_read(self._h, ctypes.byref(ms), ctypes.byref(nl),
                                                 ctypes.byref(fl), ctypes.byref(bz)))
        return ms.value, nl.value, fl.value, bz.value

    def observe_gradient_candidates(self, xs, strict=True):
        """LML and gradient of k candidate parameter vectors (rows of xs, log theta) on this GP's
        data in ONE launch sequence (gogp_observe_gradient_candidates): what Observe(xs[c]) +
        Gradient() would return for each c, without touching the GP's own state -- its factor and what was solved on it, a
        Laplace fit, its outputs and basis -- (a ShardedGP evaluates
        them one after the other in its own tiles and afterwards holds the last one's factorisation).  Counterpart:
        candidates evaluated concurrently by the reference's optimiser (optimize.Settings.
        Concurrent, tutorial/tutorial.go:30,141).  Returns (lmls[k], grads[k x P], status[k]):
        a candidate whose matrix is not positive definite has status GOGP_ENOTPD, lml NaN and a
        zero gradient instead of raising (the other candidates are still valid).  strict=False: a candidate
        with unusable parameters (status GOGP_EARG, e.g. exp(x) overflows) is reported the same way instead of
        raising -- the C ABI's per-candidate contract, on one GPU and on the shards alike."""
        xs = _arr(xs)
        P = self._ns + self._nn
        xs = xs.reshape(-1, P) if P else xs.reshape(len(xs), 0)
        k = xs.shape[0]
        self._push_data()
        lmls, grads = np.zeros(k), np.zeros((k, P))
        st = (ctypes.c_int * k)()
        rc = _lib.lib().gogp_observe_gradient_candidates(self._h, k, _dp(xs), P, _dp(lmls), _dp(grads), st)
        status = np.array(list(st), dtype=int)
        soft = (_lib.GOGP_OK, _lib.GOGP_ENOTPD, _lib.GOGP_ECOND) + (() if strict else (_lib.GOGP_EARG,))
        if rc not in soft or any(int(v) not in soft for v in status):
            self._check(rc if rc not in soft else _lib.GOGP_EARG)
        return lmls, grads, status

    # ---- batches of independent small GPs (gogp_batch_*): many members, each with its own n and theta, ONE launch ----
    def set_batch(self, X, Y, members):
        """Upload the batch data: X (rows x NDim), Y (rows) and the members, a list of (offset, n) row ranges of them
        (ranges may overlap: forecast windows are prefixes of the same data; n <= GOGP_BATCH_MAX_N).  Replaces the
        previous batch data; the GP's own data and state are not touched."""
        Xa = _arr(X).reshape(-1, self.NDim)
        Ya = _arr(Y).reshape(-1)
        if len(Xa) != len(Ya):
            raise ValueError("len(X) != len(Y)")
        mem = np.asarray(members, dtype=np.int64).reshape(-1, 2)
        off = np.ascontiguousarray(mem[:, 0])
        n = np.ascontiguousarray(mem[:, 1])
        p64 = ctypes.POINTER(ctypes.c_int64)
        self._check(_lib.lib().gogp_batch_set_data(self._h, _dp(Xa), _dp(Ya), len(Ya), len(mem),
                                                   off.ctypes.data_as(p64), n.ctypes.data_as(p64)))
        self._batch_members = len(mem)

    def _batch_args(self, xs, members):
        P = self._ns + self._nn
        xs = _arr(xs)
        xs = xs.reshape(-1, P) if P else xs.reshape(len(xs), 0)
        k = xs.shape[0]
        mem = np.arange(k) if members is None else np.asarray(members)
        mem = np.ascontiguousarray(mem.astype(np.int32).reshape(-1))
        if len(mem) != k:
            raise ValueError("len(members) != len(xs)")
        st = np.full(k, -1, dtype=np.intc)
        return xs, k, P, mem, st

    def _batch_status(self, rc, st):
        # the call itself refused (nothing evaluated: no status written) or failed: raise; per-pair outcomes
        # (GOGP_ENOTPD, GOGP_ECOND, GOGP_EARG of a non-finite row) are returned in status
        if rc != _lib.GOGP_OK and (len(st) == 0 or (st < 0).any() or
                                   rc not in (_lib.GOGP_ENOTPD, _lib.GOGP_ECOND, _lib.GOGP_EARG)):
            self._check(rc)
        return st.astype(int)

    def batch_observe_gradient(self, xs, members=None):
        """LML and gradient of k (member, log theta) pairs -- rows of xs, member members[i] (default: member i) -- in
        ONE launch (gogp_batch_observe_gradient): what Observe(xs[i]) + Gradient() on a GP holding that member's data
        would return.  Returns (lmls[k], grads[k x P], status[k]); a pair whose matrix is not positive definite has
        status GOGP_ENOTPD, lml NaN and a zero gradient, one with non-finite parameters GOGP_EARG."""
        xs, k, P, mem, st = self._batch_args(xs, members)
        lmls, grads = np.zeros(k), np.zeros((k, P))
        ip = ctypes.POINTER(ctypes.c_int)
        rc = _lib.lib().gogp_batch_observe_gradient(self._h, k, mem.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                    _dp(xs), P, _dp(lmls), _dp(grads), st.ctypes.data_as(ip))
        return lmls, grads, self._batch_status(rc, st)

    def batch_produce(self, xs, Zs, members=None):
        """LML at xs[i] and the forecasts at the test points Zs[i] (an array of rows) of k (member, log theta) pairs in
        ONE launch (gogp_batch_produce): what Observe(xs[i]) + Produce(Zs[i]) on a GP holding that member's data would
        give.  Returns (lmls[k], [mu_i], [sigma_i], status[k]); NaN where the status is GOGP_ENOTPD or GOGP_EARG."""
        xs, k, P, mem, st = self._batch_args(xs, members)
        Zl = [_arr(z).reshape(-1, self.NDim) for z in Zs]
        if len(Zl) != k:
            raise ValueError("len(Zs) != len(xs)")
        zoff = np.zeros(k + 1, dtype=np.int64)
        zoff[1:] = np.cumsum([len(z) for z in Zl])
        Z = np.ascontiguousarray(np.concatenate(Zl, axis=0)) if k else np.zeros((0, self.NDim))
        m = int(zoff[-1])
        lmls, mu, sigma = np.zeros(k), np.zeros(m), np.zeros(m)
        ip = ctypes.POINTER(ctypes.c_int)
        rc = _lib.lib().gogp_batch_produce(self._h, k, mem.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(xs), P,
                                           zoff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(Z), _dp(lmls),
                                           _dp(mu), _dp(sigma), st.ctypes.data_as(ip))
        status = self._batch_status(rc, st)
        return (lmls, [mu[zoff[i]:zoff[i + 1]] for i in range(k)], [sigma[zoff[i]:zoff[i + 1]] for i in range(k)],
                status)

    # ---- the full Observe form of the batch: every pair carries its observations in its own vector -------------------
    def _batch_full_args(self, xs):
        xl = [_arr(x).reshape(-1) for x in xs]
        k = len(xl)
        xoff = np.zeros(k + 1, dtype=np.int64)
        xoff[1:] = np.cumsum([v.size for v in xl])
        x = np.ascontiguousarray(np.concatenate(xl)) if k else np.zeros(0)
        if x.size == 0:
            x = np.zeros(1)  # (never read: a valid pointer for the call)
        return x, xoff, k, np.full(k, -1, dtype=np.intc)

    def batch_observe_full_gradient(self, xs):
        """LML and gradient of k GPs that carry their observations in their own vectors, xs[i] = [log theta | X_i | y_i]
        (lengths differ; n_i <= GOGP_BATCH_MAX_N), in ONE launch (gogp_batch_observe_full_gradient): what
        Observe(xs[i]) + Gradient() on a GP of its own would return.  Returns (lmls[k], [grad_i], status[k]); a pair
        whose matrix is not positive definite has status GOGP_ENOTPD, lml NaN and a zero gradient; a bad length,
        n_i > GOGP_BATCH_MAX_N or non-finite entries GOGP_EARG.  The GP's own data and state are not touched."""
        x, xoff, k, st = self._batch_full_args(xs)
        lmls, grads = np.zeros(k), np.zeros(x.size)
        rc = _lib.lib().gogp_batch_observe_full_gradient(self._h, k, _dp(x),
                                                         xoff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(lmls),
                                                         _dp(grads), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return lmls, [grads[xoff[i]:xoff[i + 1]] for i in range(k)], self._batch_status(rc, st)

    def batch_produce_full(self, xs, Zs):
        """LML at xs[i] (full Observe form) and the forecasts at the test points Zs[i] in ONE launch
        (gogp_batch_produce_full): what Observe(xs[i]) + Produce(Zs[i]) on a GP of its own would give.  Returns
        (lmls[k], [mu_i], [sigma_i], status[k]); NaN where the status is GOGP_ENOTPD or GOGP_EARG."""
        x, xoff, k, st = self._batch_full_args(xs)
        Zl = [_arr(z).reshape(-1, self.NDim) for z in Zs]
        if len(Zl) != k:
            raise ValueError("len(Zs) != len(xs)")
        zoff = np.zeros(k + 1, dtype=np.int64)
        zoff[1:] = np.cumsum([len(z) for z in Zl])
        Z = np.ascontiguousarray(np.concatenate(Zl, axis=0)) if k else np.zeros((0, self.NDim))
        m = int(zoff[-1])
        lmls, mu, sigma = np.zeros(k), np.zeros(m), np.zeros(m)
        p64 = ctypes.POINTER(ctypes.c_int64)
        rc = _lib.lib().gogp_batch_produce_full(self._h, k, _dp(x), xoff.ctypes.data_as(p64), zoff.ctypes.data_as(p64),
                                                _dp(Z), _dp(lmls), _dp(mu), _dp(sigma),
                                                st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        status = self._batch_status(rc, st)
        return (lmls, [mu[zoff[i]:zoff[i + 1]] for i in range(k)], [sigma[zoff[i]:zoff[i + 1]] for i in range(k)],
                status)

    def profile_read_launches(self):
        """Per launch of the tile kernel since profile_enable(True): arrays (start ms, end ms, flops, tag);
        tag = mode * 1e8 + (K / 16) * 1e5 + tiles.  Call before profile_read (which resets)."""
        L = _lib.lib()
        n = ctypes.c_int64(0)
        self._check(L.gogp_profile_read_launches(self._h, 0, None, None, None, None, ctypes.byref(n)))
        k = int(n.value)
        t0, t1, fl = np.zeros(k), np.zeros(k), np.zeros(k)
        tag = np.zeros(k, dtype=np.int64)
        if k:
            self._check(L.gogp_profile_read_launches(self._h, k, _dp(t0), _dp(t1), _dp(fl),
                                                     tag.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                     ctypes.byref(n)))
        return t0, t1, fl, tag

    def profile_read_aux(self, cls: int):
        """(sum of durations ms, timed launch groups) of one O(N^2) kernel class:
        0 Gram build, 1 gradient reduction, 2 cross-covariance (Produce)."""
        ms, nl = ctypes.c_double(0), ctypes.c_int64(0)
        self._check(_lib.lib().gogp_profile_read_aux(self._h, int(cls), ctypes.byref(ms), ctypes.byref(nl)))
        return ms.value, nl.value


def observe_gradient_batch(gps: Sequence[GP], xs) -> tuple:
    """Observe(xs[i]) + Gradient() on gps[i] for all i at once (hyperparameters-only form;
    every GP holds its own copy of the data): the k evaluations overlap on the GPU.
    Counterpart: candidates evaluated concurrently by the reference's optimiser
    (optimize.Settings.Concurrent = NTASKS, tutorial/tutorial.go:30,141).
    Returns (lmls[k], grads[k x P])."""
    k = len(gps)
    xs = _arr(xs).reshape(k, -1)
    P = xs.shape[1]
    for g in gps:
        if P != g._ns + g._nn:
            raise ValueError("len(x)")
        g._push_data()
        g._with_obs = False
    hs = (ctypes.c_void_p * k)(*[g._h for g in gps])
    lmls, grads = np.zeros(k), np.zeros((k, P))
    st = (ctypes.c_int * k)()
    rc = _lib.lib().gogp_observe_gradient_batch(hs, k, _dp(xs), P, _dp(lmls), _dp(grads), st)
    for i, g in enumerate(gps):
        if st[i] != _lib.GOGP_OK:
            g._check(st[i])
        theta = np.exp(xs[i])
        g.ThetaSimil, g.ThetaNoise = list(theta[:g._ns]), list(theta[g._ns:])
        g._last_len = P
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "observe_gradient_batch")
    return lmls, grads


class Model:
    """gp.Model (gp/model.go:9-28): GP plus priors on the hyperparameters.
    ``Priors`` is any object with Observe(x) -> float and Gradient() -> array."""

    def __init__(self, gp: GP, Priors):
        self.GP = gp
        self.Priors = Priors
        self._gGrad = None
        self._pGrad = None

    def Observe(self, x) -> float:
        gll = self.GP.Observe(x)
        self._gGrad = self.GP.Gradient()
        pll = self.Priors.Observe(x)
        self._pGrad = np.asarray(self.Priors.Gradient(), dtype=float)
        return gll + pll

    def Gradient(self) -> np.ndarray:
        g = self._gGrad.copy()
        g[:len(self._pGrad)] += self._pGrad
        return g


class LOOModel:
    """Model with the leave-one-out cross-validation score in the place of the LML: Observe(x) runs gp.Observe(x) and
    returns GP.LOOScore() (+ the log prior), Gradient() returns GP.LOOGradient() (+ the prior's).  optimize.lbfgs and
    optimize.Adam.Step then fit the hyperparameters (x = log theta, no observations in x) to the LOO objective.  The
    batched line search (``line_search_candidates`` > 1) evaluates the LML and is not offered: the GP is ``gp`` here,
    not ``GP``."""

    def __init__(self, gp: GP, Priors=None):
        self.gp = gp
        self.Priors = Priors
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the LOO objective takes the hyperparameters only")
        self.gp.Observe(self._x)
        v = self.gp.LOOScore()
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.LOOGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class HeteroscedasticModel:
    """Model whose per-observation noise variances come from a log-linear noise model fitted with the
    hyperparameters: x = [log theta (P) | phi (q)], v = exp(G phi) with ``G`` an n x q design matrix -- one-hot columns
    give one noise level per instrument, a column of ones plus time a drifting level.  Observe(x) sets v
    (GP.SetNoiseVariances) and runs gp.Observe(log theta); Gradient() returns [gp.Gradient() | G^T (v o dv)] with dv
    = GP.NoiseVariancesGradient().  ``Priors`` (Observe / Gradient over the first entries of x) is added as in Model.
    For optimize.lbfgs and optimize.Adam.Step with the sequential drivers only: the candidates path refuses
    variances (the GP is ``gp`` here, not ``GP``)."""

    def __init__(self, gp: GP, G, Priors=None):
        self.gp = gp
        self.G = _arr(G)
        if self.G.ndim != 2:
            raise ValueError("G: an n x q matrix")
        self.Priors = Priors
        self._x = None
        self._v = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        P, (n, q) = self.gp._ns + self.gp._nn, self.G.shape
        if self._x.size != P + q:
            raise ValueError("len(x): the hyperparameters and one coefficient per column of G")
        if n != len(self.gp.Y):
            raise ValueError("G: one row per observation")
        self._v = np.exp(self.G @ self._x[P:])
        self.gp.SetNoiseVariances(self._v)
        v = self.gp.Observe(self._x[:P])
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = np.concatenate([self.gp.Gradient(), self.G.T @ (self._v * self.gp.NoiseVariancesGradient())])
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class LaplaceModel:
    """Model with the Laplace approximation's log marginal likelihood under the likelihood ``lik`` ("bernoulli" /
    "poisson") in the place of the LML: Observe(x) returns GP.LaplaceObserve(x, lik) (+ the log prior), Gradient()
    GP.LaplaceGradient() (+ the prior's).  optimize.lbfgs and optimize.Adam.Step then fit x = log theta.  Sets the
    option "laplace_warm": every evaluation starts Newton's iteration from the previous mode.  As with LOOModel the
    batched line search is not offered: the GP is ``gp`` here, not ``GP``."""

    def __init__(self, gp: GP, lik, Priors=None):
        self.gp = gp
        self.lik = _lik(lik)
        self.Priors = Priors
        self._x = None
        gp.set_option("laplace_warm", 1)

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        v = self.gp.LaplaceObserve(self._x, self.lik)
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.LaplaceGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class BlockCVModel:
    """LOOModel with the leave-block-out score of GP.BlockCVScore(start) in the place of the LOO score: Observe(x) runs
    gp.Observe(x) and returns the score (+ the log prior), Gradient() returns GP.BlockCVGradient(start) (+ the
    prior's).  ``start`` is fixed at construction (``blocks(n, length)`` for equal blocks).  As with LOOModel the
    batched line search is not offered: the GP is ``gp`` here, not ``GP``."""

    def __init__(self, gp: GP, start, Priors=None):
        self.gp = gp
        self.start = _starts(start).copy()
        self.Priors = Priors
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the block cross-validation objective takes the hyperparameters only")
        self.gp.Observe(self._x)
        v = self.gp.BlockCVScore(self.start)
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.BlockCVGradient(self.start)
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class MultiModel:
    """Model with the sum of the LML of the T output columns of GP.SetOutputs in the place of the LML: Observe(x) runs
    gp.Observe(x) and returns GP.MultiLML()'s total (+ the log prior, counted once), Gradient() returns
    GP.MultiGradient() (+ the prior's).  optimize.lbfgs and optimize.Adam.Step then fit the shared hyperparameters
    (x = log theta, no observations in x) to all outputs at the price of one factorisation per evaluation.  As with
    LOOModel the batched line search is not offered: the GP is ``gp`` here, not ``GP``."""

    def __init__(self, gp: GP, Priors=None):
        self.gp = gp
        self.Priors = Priors
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the multi-output objective takes the hyperparameters only")
        self.gp.Observe(self._x)
        v = self.gp.MultiLML()[0]
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.MultiGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class BasisModel:
    """Model with GP.BasisLML in the place of the LML: Observe(x) runs gp.Observe(x) and returns GP.BasisLML() (+ the log
    prior), Gradient() returns GP.BasisGradient() (+ the prior's).  optimize.lbfgs and optimize.Adam.Step then fit the
    hyperparameters (x = log theta, no observations in x) with the coefficients of the mean of GP.SetBasis integrated
    out.  As with MultiModel the batched line search is not offered: the GP is ``gp`` here, not ``GP``."""

    def __init__(self, gp: GP, Priors=None):
        self.gp = gp
        self.Priors = Priors
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the basis objective takes the hyperparameters only")
        self.gp.Observe(self._x)
        v = self.gp.BasisLML()
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.BasisGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class SparseMultiModel:
    """SparseModel with the sum of the bounds of the T output columns of GP.SetSparseOutputs in the place of the bound:
    Observe(x) returns GP.SparseMultiObserve(x)'s total (+ the log prior, counted once), Gradient() returns
    GP.SparseMultiGradient() (+ the prior's); ``inducing=True`` as in SparseModel, with GP.SparseMultiGradientInducing()."""

    def __init__(self, gp: GP, Priors=None, inducing=False):
        self.gp = gp
        self.Priors = Priors
        self.inducing = bool(inducing)
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        p = self.gp._ns + self.gp._nn
        if self.inducing:
            m = self.gp._sparse_m
            if self._x.size != p + m * self.gp.NDim:
                raise ValueError("len(x): the sparse multi-output objective with inducing points takes the "
                                 "hyperparameters and M x NDim coordinates")
            self.gp.SetInducing(self._x[p:].reshape(m, self.gp.NDim))
        elif self._x.size != p:
            raise ValueError("len(x): the sparse multi-output objective takes the hyperparameters only")
        v = self.gp.SparseMultiObserve(self._x[:p])[0]
        return v + self.Priors.Observe(self._x[:p]) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        if self.inducing:
            g, du = self.gp.SparseMultiGradientInducing()
            g = np.concatenate([g, du.reshape(-1)])
        else:
            g = self.gp.SparseMultiGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x[:self.gp._ns + self.gp._nn])
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class CGModel:
    """Model with the iterative exact GP's estimate of the LML in the place of the LML: Observe(x) returns
    GP.CGObserve(x, probes, seed, rank, tol) on the data of GP.SetCG (+ the log prior), Gradient() returns GP.CGGradient()
    (+ the prior's), for optimize.lbfgs and optimize.Adam.  The probes are fixed by ``seed``: every x sees the same
    normals (common random numbers), so the objective is a deterministic function of x.

    With fixed probes the value and the gradient are each unbiased, but the gradient is NOT the exact derivative of the
    quadrature value: the value estimates log|K^| by Lanczos quadrature, the gradient estimates tr(K^^-1 dK^) from the
    solves.  A line search sees an inconsistency of order 1 / sqrt(probes) between the two, so optimize.Adam, which
    uses the gradient alone, is the recommended driver; lbfgs may stop early in its line search."""

    def __init__(self, gp: GP, probes: int = 16, seed: int = 0, rank: int = 64, tol: float = 1e-8, Priors=None,
                 max_iter: int = 1000):
        self.gp = gp
        self.probes, self.seed, self.rank, self.tol, self.max_iter = int(probes), int(seed), int(rank), float(tol), int(max_iter)
        self.Priors = Priors
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the iterative objective takes the hyperparameters only")
        v = self.gp.CGObserve(self._x, probes=self.probes, seed=self.seed, rank=self.rank, tol=self.tol,
                              max_iter=self.max_iter)
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.CGGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class VecchiaModel:
    """Model with Vecchia's approximation of GP.SetVecchia in the place of the LML: Observe(x) returns
    GP.VecchiaObserve(x) (+ the log prior), Gradient() returns GP.VecchiaGradient() (+ the prior's), for optimize.lbfgs and
    optimize.Adam.  The gradient is the exact derivative of the value, so a line search is consistent.  The neighbour
    table is fixed by GP.SetVecchia: a table built with length scales (vecchia.nearest) is not rebuilt as they move.

    ``lengths_of``, a callable from x = log theta to the length scales (a scalar or one per dimension), offers
    ``reneighbour(x)``: the resident table rebuilt on the device under lengths_of(x) (GP.VecchiaReneighbour), between two
    runs of an optimiser -- never inside one, where it would change the objective under the line search."""

    def __init__(self, gp: GP, Priors=None, lengths_of=None):
        self.gp = gp
        self.Priors = Priors
        self.lengths_of = lengths_of
        self._x = None

    def reneighbour(self, x) -> None:
        if self.lengths_of is None:
            raise ValueError("reneighbour: the model was built without lengths_of")
        self.gp.VecchiaReneighbour(self.lengths_of(_arr(x).reshape(-1)))

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        if self._x.size != self.gp._ns + self.gp._nn:
            raise ValueError("len(x): the Vecchia objective takes the hyperparameters only")
        v = self.gp.VecchiaObserve(self._x)
        return v + self.Priors.Observe(self._x) if self.Priors is not None else v

    def Gradient(self) -> np.ndarray:
        g = self.gp.VecchiaGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x)
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


class SparseModel:
    """Model with the collapsed bound of GP.SetSparse in the place of the LML: Observe(x) returns GP.SparseObserve(x)
    (+ the log prior), Gradient() returns GP.SparseGradient() (+ the prior's).  optimize.lbfgs and optimize.Adam.Step
    then maximise the bound over x = log theta.  As with LOOModel the batched line search is not offered: the GP is
    ``gp`` here, not ``GP``.

    ``inducing=True`` learns the inducing points too: x = [log theta (P) | U row-major (M * NDim)], with M of the last
    GP.SetSparse.  Observe moves the inducing points (GP.SetInducing) and evaluates the bound, Gradient returns
    GP.SparseGradientInducing()'s two parts in that order (the priors are on the hyperparameters alone)."""

    def __init__(self, gp: GP, Priors=None, inducing=False):
        self.gp = gp
        self.Priors = Priors
        self.inducing = bool(inducing)
        self._x = None

    def Observe(self, x) -> float:
        self._x = _arr(x).reshape(-1).copy()
        p = self.gp._ns + self.gp._nn
        if self.inducing:
            m = self.gp._sparse_m
            if self._x.size != p + m * self.gp.NDim:
                raise ValueError("len(x): the sparse objective with inducing points takes the hyperparameters and "
                                 "M x NDim coordinates")
            self.gp.SetInducing(self._x[p:].reshape(m, self.gp.NDim))
        elif self._x.size != p:
            raise ValueError("len(x): the sparse objective takes the hyperparameters only")
        v = self.gp.SparseObserve(self._x[:p])
        return v + self.Priors.Observe(self._x[:p]) if self.Priors is not None else v

    def reselect(self, x, tol=None) -> np.ndarray:
        """Re-select the inducing points among the rows of the sparse data at x = log theta (the first P entries of x) by
        GP.SelectInducing's resident form and move them there (GP.SetInducing); returns the rows taken.  The number of
        inducing points is fixed by GP.SetSparse: where the selection stops short of it, this raises and changes nothing.
        An explicit call only -- the model never re-selects by itself; an Observe has to follow."""
        p = self.gp._ns + self.gp._nn
        m = self.gp._sparse_m
        if m < 1:
            raise GogpError(_lib.GOGP_ESTATE, "reselect before SetSparse")
        idx, U, _, _ = self.gp.SelectInducing(_arr(x).reshape(-1)[:p], m, X=None, tol=tol)
        if len(idx) < m:
            raise GogpError(_lib.GOGP_ESTATE, "reselect: the selection stopped at %d of the %d inducing points of SetSparse; "
                            "they stay as they were" % (len(idx), m))
        self.gp.SetInducing(U)
        return idx

    def Gradient(self) -> np.ndarray:
        if self.inducing:
            g, du = self.gp.SparseGradientInducing()
            g = np.concatenate([g, du.reshape(-1)])
        else:
            g = self.gp.SparseGradient()
        if self.Priors is not None:
            self.Priors.Observe(self._x[:self.gp._ns + self.gp._nn])
            pg = np.asarray(self.Priors.Gradient(), dtype=float)
            g[:len(pg)] += pg
        return g


def mfma_f64_peak(iters: int = 20000, device: int = -1, details: bool = False):
    """fp64 MFMA issue-rate microbenchmark used to calibrate the roofline:
    TFLOP/s, or (TFLOP/s, cycles per MFMA on one SIMD, shader clock MHz)."""
    v, c, m = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = _lib.hooks().gogp_mfma_f64_peak(device, iters, ctypes.byref(v), ctypes.byref(c),
                                       ctypes.byref(m))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "mfma_f64_peak")
    return (v.value, c.value, m.value) if details else v.value


def mfma_f32_peak(iters: int = 20000, device: int = -1, details: bool = False):
    """The same microbenchmark for the fp32 path's v_mfma_f32_32x32x2_f32."""
    v, c, m = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = _lib.hooks().gogp_mfma_f32_peak(device, iters, ctypes.byref(v), ctypes.byref(c), ctypes.byref(m))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "mfma_f32_peak")
    return (v.value, c.value, m.value) if details else v.value


def dgemm_nt_check(A: np.ndarray, B: np.ndarray, C: np.ndarray, alpha=1.0, beta=0.0,
                  device: int = -1) -> np.ndarray:
    """C = beta*C + alpha*A@B.T on the GPU tile kernel (test hook)."""
    A, B = _arr(A), _arr(B)
    out = _arr(C).copy()
    M, K = A.shape
    N = B.shape[0]
    rc = _lib.hooks().gogp_test_dgemm_nt(device, M, N, K, alpha, _dp(A), _dp(B), beta, _dp(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_dgemm_nt")
    return out


def diag256_check(A: np.ndarray, device: int = -1):
    """Factor + invert one 256x256 SPD block on the diagonal-block kernel (test /
    diagnostic hook): returns (L, Linv, stamps[24], elapsed_us)."""
    A = _arr(A)
    assert A.shape == (256, 256)
    L, X = np.zeros((256, 256)), np.zeros((256, 256))
    st = (ctypes.c_uint64 * 32)()
    us = ctypes.c_double(0.0)
    rc = _lib.hooks().gogp_test_diag256(device, _dp(A), _dp(L), _dp(X), st, ctypes.byref(us))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_diag256")
    return L, X, np.array(list(st), dtype=np.uint64), us.value


def bench_gemm(mode: int, mt: int, nt: int, K: int, reps: int = 5, device: int = -1):
    """Time the tile kernel on one shape: returns (ms per launch, TFLOP/s)."""
    ms, tf = ctypes.c_double(0.0), ctypes.c_double(0.0)
    rc = _lib.hooks().gogp_bench_gemm(device, mode, mt, nt, K, reps, ctypes.byref(ms), ctypes.byref(tf))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "bench_gemm")
    return ms.value, tf.value


GEMM_MODES = {"RECT": 0, "LOWER": 1, "LAUUM": 2, "TRAP": 3}


def _covers(n, off, ld, rows, cols, k, stride, what):
    # the launch addresses off + c * stride + r * ld + [0, cols) for c < k, r < rows
    if off < 0 or ld < cols or stride < 0 or off + (k - 1) * stride + (rows - 1) * ld + cols > n:
        raise ValueError("%s: %d elements do not cover off %d, ld %d, %d x %d, %d slots %d apart"
                         % (what, n, off, ld, rows, cols, k, stride))


def gemm_nt_check(mode, mt: int, nt: int, K: int, A: np.ndarray, B: np.ndarray, C: np.ndarray, alpha=1.0, beta=0.0,
                  lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=0, device: int = -1, **opts) -> np.ndarray:
    """The product launcher of the tile kernel (test hook gogp_test_gemm_nt) on host arrays: returns a copy of the
    whole of C after  C = beta C + alpha A B^T  over mt x nt tiles of 128 in `mode` (RECT, LOWER, LAUUM, TRAP or
    0..3).  The dtype (float64 / float32, the same for all three) picks the kernel.  The arrays are taken flat; the
    launch sees them at element offsets a_off, b_off, c_off with leading dimensions lda, ldb, ldc (default: the
    arrays' row length).  opts: the GemmGrid fields of _lib.CGemmOpts, plus k candidates bstride elements apart.
    Every array must cover what the launch addresses (ValueError otherwise, before the hook is called)."""
    mode = GEMM_MODES.get(mode, mode)
    arrs = []
    for a in (A, B, C):
        if not isinstance(a, np.ndarray) or a.dtype not in (np.float64, np.float32) or not a.flags.c_contiguous:
            raise TypeError("operands: C-contiguous float64 / float32 arrays")
        arrs.append(a)
    if len({a.dtype for a in arrs}) != 1:
        raise TypeError("A, B and C must share one dtype")
    prec = 64 if A.dtype == np.float64 else 32
    lda = A.shape[-1] if lda is None else lda
    ldb = B.shape[-1] if ldb is None else ldb
    ldc = C.shape[-1] if ldc is None else ldc
    o = dict(_lib.CGemmOpts.DEFAULTS)
    unknown = set(opts) - set(o)
    if unknown:
        raise TypeError("unknown options %s" % sorted(unknown))
    o.update(opts)
    k, bstride = o["k"], o["bstride"]
    rows_b = mt if mode in (1, 2) else nt
    _covers(A.size, a_off, lda, mt * 128, K, k, bstride, "A")
    _covers(B.size, b_off, ldb, rows_b * 128, K, k, bstride, "B")
    _covers(C.size, c_off, ldc, mt * 128, nt * 128, k, bstride, "C")
    out = C.copy()
    copt = _lib.CGemmOpts(**o)
    rc = _lib.hooks().gogp_test_gemm_nt(device, prec, mode, mt, nt, K, alpha, beta,
                                        A.ctypes.data, A.size, a_off, lda, B.ctypes.data, B.size, b_off, ldb,
                                        out.ctypes.data, out.size, c_off, ldc, ctypes.byref(copt))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_gemm_nt")
    return out


def diag_syrk_check(L: np.ndarray, D64: np.ndarray, K: int, nblocks: int, bs: int = 256, ld=None, l_off: int = 0,
                    row_stride=None, device: int = -1) -> np.ndarray:
    """The fp32 path's fp64 diagonal-block update (test hook gogp_test_diag_syrk): returns a copy of the whole of D64
    after  D64 block b -= R_b R_b^T  (b < nblocks), R_b the bs x K floats of L at l_off + b * row_stride, leading
    dimension ld.  bs = 256 is the single-GPU launcher (row_stride = 256 ld), 512 the sharded one."""
    if L.dtype != np.float32 or D64.dtype != np.float64 or not (L.flags.c_contiguous and D64.flags.c_contiguous):
        raise TypeError("L: float32, D64: float64, both C-contiguous")
    ld = L.shape[-1] if ld is None else ld
    row_stride = bs * ld if row_stride is None else row_stride
    _covers(L.size, l_off, ld, bs, K, nblocks, row_stride, "L")
    if D64.size < nblocks * bs * bs:
        raise ValueError("D64 holds fewer than %d blocks" % nblocks)
    out = D64.copy()
    rc = _lib.hooks().gogp_test_diag_syrk(device, bs, L.ctypes.data, L.size, l_off, ld, K, row_stride, _dp(out),
                                          out.size, nblocks)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_diag_syrk")
    return out


def diag256_product(A: np.ndarray, variant: int = 0, row0: int = 0, nvalid: int = 256, L=None, Dinv=None,
                    device: int = -1):
    """The product build of the diagonal-block kernel (test hook gogp_test_diag256_product) on one 256 x 256 block:
    variant 0 factor + inverse, 1 the same with Dinv of leading dimension 512, 2 inverse only (A holds the factor),
    3 inverse only at 512.  A: 256 rows (its row length is the leading dimension).  L (256 x ldl) and Dinv
    (256 x 256 | 512) are the outputs' initial contents (zeros by default).  Returns (L, Dinv, info)."""
    A = _arr(A)
    if A.ndim != 2 or A.shape[0] != 256 or A.shape[1] < 256:
        raise ValueError("A: 256 rows of at least 256")
    L = np.zeros((256, 256)) if L is None else _arr(L).copy()
    ldd = 512 if variant in (1, 3) else 256
    Dinv = np.zeros((256, ldd)) if Dinv is None else _arr(Dinv).copy()
    if L.ndim != 2 or L.shape[0] != 256 or L.shape[1] < 256 or Dinv.shape != (256, ldd):
        raise ValueError("L: 256 rows of at least 256, Dinv: 256 x %d" % ldd)
    info = ctypes.c_longlong(0)
    rc = _lib.hooks().gogp_test_diag256_product(device, variant, _dp(A), A.shape[1], _dp(L), L.shape[1], _dp(Dinv),
                                                row0, nvalid, ctypes.byref(info))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_diag256_product")
    return L, Dinv, info.value


# ---- the kernels that consume the factor (include/gogp_testhooks.h; tests/test_substitution_kernels.py) ------------
def _mat(a, what):
    if not isinstance(a, np.ndarray) or a.dtype not in (np.float64, np.float32) or not a.flags.c_contiguous:
        raise TypeError("%s: a C-contiguous float64 / float32 array" % what)
    return a


def _prec(*arrs):
    if len({a.dtype for a in arrs}) != 1:
        raise TypeError("the matrices must share one dtype")
    return 64 if arrs[0].dtype == np.float64 else 32


def _vec(a, what):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
        raise TypeError("%s: a C-contiguous float64 array" % what)
    return a


def trsm_small_workspace(npad: int) -> int:
    """Bytes of the workspace of one launch of the one-pass substitution."""
    n = _lib.hooks().gogp_test_trsm_small_workspace(npad)
    if n < 0:
        raise GogpError(_lib.GOGP_EARG, "test_trsm_small_workspace")
    return int(n)


def trsm_small_check(npad: int, L: np.ndarray, ld: int, Dinv: np.ndarray, KsT: np.ndarray, ldk: int, j0: int, cnt: int,
                     dq: np.ndarray, ws=None, device: int = -1):
    """One launch_trsm_small (test hook gogp_test_trsm_small) on flat host arrays.  ws: the workspace's initial bytes
    (uint8, trsm_small_workspace(npad) of them; default zeros).  Returns (dq, ws, kind, width, sol_off, tmo): copies of
    dq and of the whole workspace after the launch, what trsm_small_solution reports, and the time-out word."""
    L, Dinv, KsT = _mat(L, "L"), _mat(Dinv, "Dinv"), _mat(KsT, "KsT")
    prec = _prec(L, Dinv, KsT)
    if Dinv.size != npad * 256:
        raise ValueError("Dinv: npad / 256 blocks of 256 x 256")
    dq = _vec(dq, "dq").copy()
    nbytes = trsm_small_workspace(npad)
    ws = np.zeros(nbytes, np.uint8) if ws is None else np.ascontiguousarray(ws, dtype=np.uint8).copy()
    kind, width, tmo, off = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_uint(0), ctypes.c_int64(-1)
    rc = _lib.hooks().gogp_test_trsm_small(device, prec, npad, L.ctypes.data, L.size, ld, Dinv.ctypes.data,
                                           KsT.ctypes.data, KsT.size, ldk, j0, cnt, _dp(dq), dq.size, ws.ctypes.data,
                                           ws.size, ctypes.byref(kind), ctypes.byref(width), ctypes.byref(off),
                                           ctypes.byref(tmo))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_trsm_small")
    return dq, ws, kind.value, width.value, off.value, tmo.value


def trsv_steps_check(direction: str, npad: int, L: np.ndarray, ld: int, Dinv: np.ndarray, b0: int, b1: int,
                     w: np.ndarray, out: np.ndarray, k: int = 1, bstride: int = 0, device: int = -1):
    """The product's substitution steps b0 .. b1 (test hook gogp_test_trsv_steps): "fwd" ascending (out = z), "bwd"
    descending (out = alpha).  Returns copies of (w, out) after the steps."""
    L, Dinv = _mat(L, "L"), _mat(Dinv, "Dinv")
    prec = _prec(L, Dinv)
    if Dinv.size != (k - 1) * bstride + npad * 256:
        raise ValueError("Dinv: (k - 1) * bstride + npad * 256 elements")
    w, out = _vec(w, "w").copy(), _vec(out, "out").copy()
    rc = _lib.hooks().gogp_test_trsv_steps(device, prec, {"fwd": 0, "bwd": 1}[direction], npad, L.ctypes.data, L.size,
                                           ld, Dinv.ctypes.data, b0, b1, k, bstride, _dp(w), w.size, _dp(out), out.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_trsv_steps")
    return w, out


def alpha_from_y_check(npad: int, Y: np.ndarray, ld: int, z: np.ndarray, alpha: np.ndarray, device: int = -1):
    """launch_alpha_from_y (test hook gogp_test_alpha_from_y); returns a copy of alpha after the launch."""
    Y, z, alpha = _mat(Y, "Y"), _vec(z, "z"), _vec(alpha, "alpha").copy()
    rc = _lib.hooks().gogp_test_alpha_from_y(device, _prec(Y), npad, Y.ctypes.data, Y.size, ld, _dp(z), z.size,
                                             _dp(alpha), alpha.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_alpha_from_y")
    return alpha


def rownorm_dot_check(V: np.ndarray, ld: int, ncols: int, m: int, vec=None, dot=None, sq=None, device: int = -1):
    """launch_rownorm_dot (test hook gogp_test_rownorm_dot); vec, dot, sq: each None or an array.  Returns copies of
    (dot, sq) after the launch (None where None went in)."""
    V = _mat(V, "V")
    vec = None if vec is None else _vec(vec, "vec")
    dot = None if dot is None else _vec(dot, "dot").copy()
    sq = None if sq is None else _vec(sq, "sq").copy()
    size = lambda a: 0 if a is None else a.size  # noqa: E731
    rc = _lib.hooks().gogp_test_rownorm_dot(device, _prec(V), V.ctypes.data, V.size, ld, ncols, m, _dp(vec), size(vec),
                                            _dp(dot), size(dot), _dp(sq), size(sq))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_rownorm_dot")
    return dot, sq


def tinv_check(nsub: int, Dinv: np.ndarray, X: np.ndarray, tld: int, XT=None, device: int = -1):
    """launch_tinv_init (test hook gogp_test_tinv); returns copies of (X, XT) after the launch."""
    Dinv, X = _mat(Dinv, "Dinv"), _mat(X, "X").copy()
    arrs = [Dinv, X]
    if XT is not None:
        XT = _mat(XT, "XT").copy()
        arrs.append(XT)
        if XT.size != X.size:
            raise ValueError("XT: as many elements as X")
    if Dinv.size != nsub * 65536:
        raise ValueError("Dinv: nsub blocks of 256 x 256")
    rc = _lib.hooks().gogp_test_tinv(device, _prec(*arrs), nsub, Dinv.ctypes.data, X.ctypes.data, X.size, tld,
                                     int(XT is not None), None if XT is None else XT.ctypes.data)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_tinv")
    return X, XT


def blockmm_check(arena: np.ndarray, prods, alpha: float = 1.0, k: int = 1, bstride: int = 0, device: int = -1):
    """launch_blockmm (test hook gogp_test_blockmm) on one arena; prods: up to six (a_off, lda, b_off, ldb, c_off, ldc,
    K).  Returns a copy of the arena after the launch."""
    arena = _mat(arena, "arena").copy()
    n = len(prods)
    cols = [(ctypes.c_int64 * max(n, 1))(*[int(p[i]) for p in prods]) for i in range(6)]
    K = (ctypes.c_int * max(n, 1))(*[int(p[6]) for p in prods])
    rc = _lib.hooks().gogp_test_blockmm(device, _prec(arena), n, arena.ctypes.data, arena.size, *cols, K, alpha, k,
                                        bstride)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_blockmm")
    return arena


# ---- the kernels that turn K^-1 into the gradient (include/gogp_testhooks.h; tests/test_grad_kernels.py) -------------
NACC = _lib.GOGP_TEST_NACC
ACC_TRACE, ACC_ARD0 = 12, 16


def kparams(ndim: int, terms, noise_var: float = 0.0, dnoise: float = 0.0, events=(), ev_axis: int = 0):
    """A gogp_test_kparams.  terms: dicts with kind, and optionally ard (False), c (1.0), w (0.0) and inv_len (a number, or
    ndim of them for an ARD term); events: (from, to, discount) triples."""
    if not 1 <= ndim <= 64 or not 1 <= len(terms) <= 4 or len(events) > 32:
        raise ValueError("kparams: 1..64 dimensions, 1..4 terms, at most 32 events")
    p = _lib.CKParams()
    p.ndim, p.nterms, p.noise_var, p.dnoise, p.nevents, p.ev_axis = ndim, len(terms), noise_var, dnoise, len(events), ev_axis
    for t, T in enumerate(terms):
        p.kind[t], p.ard[t], p.c[t], p.w[t] = int(T["kind"]), int(bool(T.get("ard"))), T.get("c", 1.0), T.get("w", 0.0)
        il = np.broadcast_to(np.asarray(T.get("inv_len", 1.0), float), (ndim,))
        for d in range(ndim):
            p.inv_len[t][d] = il[d]
    for e, (frm, to, disc) in enumerate(events):
        p.ev_from[e], p.ev_to[e], p.ev_disc[e] = frm, to, disc
    return p


def grad_blocks(npad: int, max_blocks: int = 0, mrows: int = 0, ncols: int = 0) -> int:
    """Workgroups (rows of `partials`) of launch_grad_reduce, or with mrows, ncols of launch_grad_reduce_local."""
    b = _lib.hooks().gogp_test_grad_blocks(npad, mrows, ncols, max_blocks)
    if b < 0:
        raise GogpError(_lib.GOGP_EARG, "test_grad_blocks")
    return int(b)


def _kp_array(kp):
    kps = list(kp) if isinstance(kp, (list, tuple)) else [kp]
    return (_lib.CKParams * len(kps))(*kps), len(kps)


def grad_reduce_check(kp, X: np.ndarray, alpha: np.ndarray, Kinv: np.ndarray, ld: int, n: int, npad: int,
                      partials: np.ndarray, out: np.ndarray, ard_dims: int = 0, radial1: bool = False, mfma_min: int = 1,
                      ev: bool = False, max_blocks: int = 0, bstride: int = 0, device: int = -1):
    """launch_grad_reduce (test hook gogp_test_grad_reduce) on flat host arrays; kp: one kparams(), or a list of k of them
    (candidates, bstride elements apart).  Returns copies of (partials, out) after the launch; out is k x NACC."""
    arr, k = _kp_array(kp)
    X, alpha, Kinv = _vec(X, "X"), _vec(alpha, "alpha"), _mat(Kinv, "Kinv")
    partials, out = _vec(partials, "partials").copy(), _vec(out, "out").copy()
    if out.size != k * NACC:
        raise ValueError("out: k x NACC")
    rc = _lib.hooks().gogp_test_grad_reduce(device, _prec(Kinv), arr, ard_dims, int(radial1), mfma_min, int(ev), _dp(X),
                                            X.size, _dp(alpha), alpha.size, Kinv.ctypes.data, Kinv.size, ld, n, npad,
                                            max_blocks, k, bstride, _dp(partials), partials.size, _dp(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_grad_reduce")
    return partials, out.reshape(k, NACC)


def grad_reduce_local_check(kp, X: np.ndarray, alpha: np.ndarray, Kinv: np.ndarray, ld: int, n: int, npad: int, mrows: int,
                            ncols: int, grid, partials: np.ndarray, out: np.ndarray, ard_dims: int = 0,
                            radial1: bool = False, mfma_min: int = 1, ev: bool = False, max_blocks: int = 0,
                            nb_shift: int = 9, device: int = -1):
    """launch_grad_reduce_local (test hook gogp_test_grad_reduce_local); grid = (pr, Pr, pc, Pc).  Returns copies of
    (partials, out) after the launch."""
    arr, k = _kp_array(kp)
    X, alpha, Kinv = _vec(X, "X"), _vec(alpha, "alpha"), _mat(Kinv, "Kinv")
    partials, out = _vec(partials, "partials").copy(), _vec(out, "out").copy()
    if out.size != NACC:
        raise ValueError("out: NACC")
    pr, Pr, pc, Pc = grid
    rc = _lib.hooks().gogp_test_grad_reduce_local(device, _prec(Kinv), arr, ard_dims, int(radial1), mfma_min, int(ev),
                                                  _dp(X), X.size, _dp(alpha), alpha.size, Kinv.ctypes.data, Kinv.size, ld,
                                                  n, npad, mrows, ncols, nb_shift, pr, Pr, pc, Pc, max_blocks, k, 0,
                                                  _dp(partials), partials.size, _dp(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_grad_reduce_local")
    return partials, out


def xgrad_check(kp, X: np.ndarray, alpha: np.ndarray, Kinv: np.ndarray, ld: int, n: int, npad: int, gx: np.ndarray,
                ev: bool = False, device: int = -1):
    """launch_xgrad (test hook gogp_test_xgrad); returns copies of (Kinv, gx) after the launch."""
    X, alpha = _vec(X, "X"), _vec(alpha, "alpha")
    Kinv, gx = _vec(Kinv, "Kinv").copy(), _vec(gx, "gx").copy()
    rc = _lib.hooks().gogp_test_xgrad(device, ctypes.byref(kp), int(ev), _dp(X), X.size, _dp(alpha), alpha.size, _dp(Kinv),
                                      Kinv.size, ld, n, npad, _dp(gx), gx.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_xgrad")
    return Kinv, gx


# ---- the kernels of Append, Remove, ProduceGradient's skinny product and ProduceCovariance (include/gogp_testhooks.h;
# tests/test_update_kernels.py) ------------------------------------------------------------------------------------------
TS_SOL_ROWS = 3


def _raw(a, what):
    if a is None:
        return None, 0
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous:
        raise TypeError("%s: a C-contiguous uint8 array" % what)
    return a.ctypes.data, a.size


def _ints(a, what):
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
        raise TypeError("%s: a C-contiguous int32 array" % what)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def append_gram_check(src0, src1, m0: int, m: int, npc: int, n: int, z: np.ndarray, part: np.ndarray, Lnew: np.ndarray,
                      ld: int, device: int = -1):
    """launch_append_gram (test hook gogp_test_append_gram).  src0, src1: (raw bytes or None, kind, width, byte offset) of
    the two sources of V.  Returns copies of (part, Lnew) after the launch."""
    (r0, k0, w0, o0), (r1, k1, w1, o1) = src0, src1
    p0, n0 = _raw(r0, "src0")
    p1, n1 = _raw(r1, "src1")
    z, part, Lnew = _vec(z, "z"), _vec(part, "part").copy(), _vec(Lnew, "Lnew").copy()
    rc = _lib.hooks().gogp_test_append_gram(device, p0, n0, k0, w0, o0, p1, n1, k1, w1, o1, m0, m, npc, n, _dp(z), z.size,
                                            _dp(part), part.size, _dp(Lnew), Lnew.size, ld)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_append_gram")
    return part, Lnew


def append_commit_check(kp, X2: np.ndarray, y2: np.ndarray, m: int, n: int, part: np.ndarray, nslab: int, Lnew: np.ndarray,
                        ld: int, z2: np.ndarray, info: int = 0, ev: bool = False, device: int = -1):
    """launch_append_commit (test hook gogp_test_append_commit); returns copies of (Lnew, z2) and info after the launch."""
    X2, y2, part = _vec(X2, "X2"), _vec(y2, "y2"), _vec(part, "part")
    Lnew, z2 = _vec(Lnew, "Lnew").copy(), _vec(z2, "z2").copy()
    inf = ctypes.c_longlong(info)
    rc = _lib.hooks().gogp_test_append_commit(device, ctypes.byref(kp), int(ev), _dp(X2), X2.size, _dp(y2), y2.size, m, n,
                                              _dp(part), part.size, nslab, _dp(Lnew), Lnew.size, ld, _dp(z2), z2.size,
                                              ctypes.byref(inf))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_append_commit")
    return Lnew, z2, int(inf.value)


def nv_append_commit_check(kp, X2: np.ndarray, y2: np.ndarray, v2, m: int, n: int, part: np.ndarray, nslab: int,
                           Lnew: np.ndarray, ld: int, z2: np.ndarray, info: int = 0, ev: bool = False, device: int = -1):
    """append_commit_check with the new rows' noise variances v2 folded into the parts first (launch_nv_append_fold, as
    gogp_append_noisy; test hook gogp_test_nv_append_commit).  v2 = None: launch_append_commit alone.  Returns copies of
    (Lnew, z2), info and the parts after the launches."""
    X2, y2, part = _vec(X2, "X2"), _vec(y2, "y2"), _vec(part, "part").copy()
    v2 = None if v2 is None else _vec(v2, "v2")
    Lnew, z2 = _vec(Lnew, "Lnew").copy(), _vec(z2, "z2").copy()
    inf = ctypes.c_longlong(info)
    rc = _lib.hooks().gogp_test_nv_append_commit(device, ctypes.byref(kp), int(ev), _dp(X2), X2.size, _dp(y2), y2.size,
                                                 _dp(v2), 0 if v2 is None else v2.size, m, n, _dp(part), part.size, nslab,
                                                 _dp(Lnew), Lnew.size, ld, _dp(z2), z2.size, ctypes.byref(inf))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_nv_append_commit")
    return Lnew, z2, int(inf.value), part


def remove_gather_check(src: np.ndarray, ld0: int, map_: np.ndarray, n1: int, dst: np.ndarray, npad1: int,
                        device: int = -1):
    """launch_remove_gather (test hook gogp_test_remove_gather); returns a copy of dst after the launch."""
    src, dst = _vec(src, "src"), _vec(dst, "dst").copy()
    rc = _lib.hooks().gogp_test_remove_gather(device, _dp(src), src.size, ld0, _ints(map_, "map"), map_.size, n1, _dp(dst),
                                              dst.size, npad1)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_remove_gather")
    return dst


def remove_w_check(src: np.ndarray, ld0: int, map_: np.ndarray, rem: np.ndarray, mc: int, mw: int, r0: int, n1: int,
                   npad1: int, W: np.ndarray, device: int = -1):
    """launch_remove_w (test hook gogp_test_remove_w); returns a copy of W after the launch."""
    src, W = _vec(src, "src"), _vec(W, "W").copy()
    rc = _lib.hooks().gogp_test_remove_w(device, _dp(src), src.size, ld0, _ints(map_, "map"), map_.size, _ints(rem, "rem"),
                                         rem.size, mc, mw, r0, n1, npad1, _dp(W), W.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_remove_w")
    return W


def remove_block_check(L: np.ndarray, ld: int, W: np.ndarray, mw: int, kb0: int, kb1: int, n1: int, snap: np.ndarray,
                       snap_b0: int, snap_nb: int, device: int = -1):
    """launch_remove_snap (blocks snap_b0 .. snap_b0 + snap_nb - 1), then launch_remove_block for kb = kb0, kb0 + 128, ..,
    kb1 (test hook gogp_test_remove_block).  Returns copies of (L, W, snap) after the launches."""
    L, W, snap = _vec(L, "L").copy(), _vec(W, "W").copy(), _vec(snap, "snap").copy()
    rc = _lib.hooks().gogp_test_remove_block(device, _dp(L), L.size, ld, snap_b0, snap_nb, _dp(snap), snap.size, _dp(W),
                                             W.size, mw, kb0, kb1, n1)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_remove_block")
    return L, W, snap


def bwd_panel_check(rows16: int, A: np.ndarray, a_off: int, lda: int, B: np.ndarray, b_off: int, ldb: int, C: np.ndarray,
                    c_off: int, ldc: int, ncols: int, K: int, tri: bool = False, sub: bool = False, device: int = -1):
    """launch_bwd_panel (test hook gogp_test_bwd_panel); returns a copy of C after the launch."""
    A, B, C = _vec(A, "A"), _vec(B, "B"), _vec(C, "C").copy()
    rc = _lib.hooks().gogp_test_bwd_panel(device, rows16, _dp(A), A.size, a_off, lda, _dp(B), B.size, b_off, ldb, _dp(C),
                                          C.size, c_off, ldc, ncols, K, int(tri), int(sub))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_bwd_panel")
    return C


def pcov_slabs(npad: int, m: int, ncu: int):
    """(slabs, columns per slab) of launch_pcov for ncu compute units.  No device."""
    cps = ctypes.c_int(0)
    ns = _lib.hooks().gogp_test_pcov_slabs(npad, m, ncu, ctypes.byref(cps))
    if ns < 0:
        raise GogpError(_lib.GOGP_EARG, "test_pcov_slabs")
    return int(ns), int(cps.value)


def pcov_check(kp, Z: np.ndarray, m: int, Vt, ld: int, npad: int, ncu: int, part, out: np.ndarray, mo: int, ldo: int,
               diag_add: float = 0.0, ev: bool = False, device: int = -1):
    """launch_pcov (test hook gogp_test_pcov) with the number of compute units given; Vt None: the prior Gram matrix (part
    may be None then).  Returns copies of (part, out) after the launch."""
    Z, out = _vec(Z, "Z"), _vec(out, "out").copy()
    Vt = None if Vt is None else _vec(Vt, "Vt")
    part = None if part is None else _vec(part, "part").copy()
    size = lambda a: 0 if a is None else a.size  # noqa: E731
    rc = _lib.hooks().gogp_test_pcov(device, ctypes.byref(kp), int(ev), _dp(Z), Z.size, m, _dp(Vt), size(Vt), ld, npad, ncu,
                                     _dp(part), size(part), diag_add, _dp(out), out.size, mo, ldo)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_pcov")
    return part, out


def multi_weight_check(At: np.ndarray, ld: int, T: int, Kinv: np.ndarray, ldk: int, n: int, npad: int, G: np.ndarray,
                       device: int = -1) -> np.ndarray:
    """launch_multi_weight (test hook gogp_test_multi_weight): G = T Kinv - A A^T on the elements j <= i < n of the lower
    64 x 64 tiles, zeros on the rest of them; At holds one column of A per row of ld.  Returns a copy of G after the
    launch."""
    At, Kinv, G = _vec(At, "At"), _vec(Kinv, "Kinv"), _vec(G, "G").copy()
    rc = _lib.hooks().gogp_test_multi_weight(device, _dp(At), At.size, ld, T, _dp(Kinv), Kinv.size, ldk, n, npad, _dp(G),
                                            G.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_multi_weight")
    return G


# ---- the small finishing kernels of leave-one-out, multi-output and sparse (include/gogp_testhooks.h;
# tests/test_finish_kernels.py) ----------------------------------------------------------------------------------------
def finish_check(which: str, device: int = -1, **args):
    """The test hook gogp_test_<which> of one of the launchers in _lib.FINISH_HOOKS, whose table names the arguments: flat
    float64 arrays (their lengths are passed along) and scalars, all by keyword.  Returns copies of the in / out arrays
    after the launch, in the order of the table (a single array if there is one)."""
    return _table_check(_lib.FINISH_HOOKS, which, device, args, "finish_check")


def select_blocks(N: int, max_blocks: int = 0) -> int:
    """Workgroups of a step of the greedy selection (select.hip: select_blocks): one per 256 rows, 1024 at most,
    max_blocks where that is positive and smaller.  Workgroup b owns the rows i with (i // 256) % workgroups == b."""
    nb = max(1, min((N + 255) // 256, 1024))
    return max_blocks if 0 < max_blocks < nb else nb


def select_step_check(kp, X: np.ndarray, N: int, Lt: np.ndarray, ldn: int, j: int, tol: float, d: np.ndarray,
                      sel: np.ndarray, part_v: np.ndarray, part_i: np.ndarray, max_blocks: int = 0, device: int = -1):
    """One step of the greedy selection (test hook gogp_test_select_step) on flat host arrays: Lt j + 1 columns of ldn
    (column-major), d (N), sel (N, uint8), the previous launch's partial maxima (values, rows).  Returns copies after the
    launch: (Lt, d, sel, out_v, out_i, p, dp), p = -1 where the step stopped."""
    X, Lt, d = _vec(X, "X"), _vec(Lt, "Lt").copy(), _vec(d, "d").copy()
    sel = np.ascontiguousarray(np.asarray(sel, dtype=np.uint8)).copy()
    part_v = _vec(part_v, "part_v")
    part_i = np.ascontiguousarray(np.asarray(part_i, dtype=np.int64))
    nb = max(part_v.size, 1)
    out_v, out_i = np.full(nb, np.nan), np.full(nb, -1, dtype=np.int64)
    p, dp = ctypes.c_int64(-2), ctypes.c_double(np.nan)
    rc = _lib.hooks().gogp_test_select_step(device, kp, _dp(X), X.size, N, _dp(Lt), Lt.size, ldn, j, tol, _dp(d), d.size,
                                            sel.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), sel.size, _dp(part_v),
                                            _ip(part_i), min(part_v.size, part_i.size), max_blocks, _dp(out_v), _ip(out_i),
                                            out_v.size, ctypes.byref(p), ctypes.byref(dp))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_select_step")
    return Lt, d, sel, out_v, out_i, p.value, dp.value


def select_run_check(kp, X: np.ndarray, N: int, M: int, tol: float, max_blocks: int = 0, d0=None, device: int = -1):
    """The whole greedy selection (test hook gogp_test_select_run) with the grid capped at max_blocks and, d0 given, d0 in
    the place of the initial diagonal.  Returns (idx, pivots, U, Lt, d, trace) cut to the m steps taken: Lt as m columns of
    N rows (column-major on the device, returned as an N x m array), d the final residuals."""
    X = _vec(X, "X")
    D = kp.ndim
    ldn = (N + 255) // 256 * 256
    cols = max(min(M, N), 1)
    idx, piv, U = np.zeros(max(M, 1), dtype=np.int64), np.zeros(max(M, 1)), np.zeros(max(M, 1) * D)
    Lt, d = np.zeros(cols * max(ldn, 1)), np.zeros(max(N, 1))
    d0a = None if d0 is None else _vec(d0, "d0")
    m, tr = ctypes.c_int64(0), ctypes.c_double(0.0)
    rc = _lib.hooks().gogp_test_select_run(device, kp, _dp(X), X.size, N, M, tol, max_blocks, _dp(d0a),
                                           0 if d0a is None else d0a.size, _ip(idx), _dp(piv), _dp(U), U.size, _dp(Lt),
                                           Lt.size, _dp(d), d.size, ctypes.byref(m), ctypes.byref(tr))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_select_run")
    k = m.value
    L = Lt.reshape(cols, max(ldn, 1))[:k, :N].T.copy()
    return idx[:k].copy(), piv[:k].copy(), U.reshape(-1, D)[:k].copy(), L, d[:N].copy(), tr.value


def laplace_kernel_check(which: str, device: int = -1, **args):
    """finish_check for the kernels of the Laplace approximation (_lib.LAPLACE_HOOKS)."""
    return _table_check(_lib.LAPLACE_HOOKS, which, device, args, "laplace_kernel_check")


def noise_variances_kernel_check(which: str, device: int = -1, **args):
    """finish_check for the kernels of the per-observation noise variances (_lib.NOISEVAR_HOOKS)."""
    return _table_check(_lib.NOISEVAR_HOOKS, which, device, args, "noise_variances_kernel_check")


def basis_kernel_check(which: str, device: int = -1, **args):
    """finish_check for the kernels of the explicit basis functions (_lib.BASIS_HOOKS)."""
    return _table_check(_lib.BASIS_HOOKS, which, device, args, "basis_kernel_check")


def shard_kernel_check(which: str, device: int = -1, **args):
    """finish_check for the kernels of the sharded path and the rest of solve.hip (_lib.SHARD_HOOKS): arrays typed by
    `precision` are float64 or float32, and the optional ones may be None."""
    return _table_check(_lib.SHARD_HOOKS, which, device, args, "shard_kernel_check")


def chunk_tdot_scratch(rows: int, nb: int) -> int:
    """Doubles of `part` scratch launch_chunk_tdot needs for up to `rows` rows.  No device."""
    r = int(_lib.hooks().gogp_test_chunk_tdot_scratch(rows, nb))
    if r < 0:
        raise GogpError(_lib.GOGP_EARG, "test_chunk_tdot_scratch")
    return r


def basis_slabs(n: int):
    """(symm, gram): the slabs launch_basis_symm and launch_basis_gram split n observations into."""
    return int(_lib.hooks().gogp_test_basis_symm_slabs(n)), int(_lib.hooks().gogp_test_basis_gram_slabs(n))


def _table_check(table, which: str, device: int, args, caller: str):
    spec = table[which]
    if set(args) != {name for name, _ in spec}:
        raise TypeError("%s(%s): the arguments are %s" % (caller, which, ", ".join(name for name, _ in spec)))
    call, outs = [device], []
    typed = {"A": "precision", "O": "precision", "P": "precision2", "B": "precision"}
    for name, kind in spec:
        v = args[name]
        if kind in "nrB" and v is None:
            call += [None, 0]
        elif kind in "AOPBfrn":  # arrays by their own element type (_lib._SHARD_SPEC)
            want = {"f": np.float32, "r": np.int64, "n": np.float64}.get(kind)
            if want is None:
                want = {64: np.float64, 32: np.float32}.get(int(args[typed[kind]]))
            if not isinstance(v, np.ndarray) or v.dtype != want or not v.flags.c_contiguous:
                raise TypeError("%s: a C-contiguous %s array" % (name, np.dtype(want).name if want else "float"))
            v = v.reshape(-1)
            if kind in "OP":
                v = v.copy()
                outs.append(v)
            call += [ctypes.c_void_p(v.ctypes.data), v.size]
        elif kind in "ao":
            v = _vec(v, name).reshape(-1)
            if kind == "o":
                v = v.copy()
                outs.append(v)
            call += [_dp(v), v.size]
        else:
            call.append(float(v) if kind == "d" else int(v))
    rc = getattr(_lib.hooks(), "gogp_test_" + which)(*call)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_" + which)
    return outs[0] if len(outs) == 1 else tuple(outs)


# ---- the kernels of gram.hip and the forecast-derivative kernels of pgrad.hip (include/gogp_testhooks.h;
# tests/test_gram_kernels.py).  Every wrapper works on flat host arrays and returns copies of the in / out arrays after the
# launch; a refusal or a device error raises GogpError.
def gram_split_check(kp, X: np.ndarray, n: int, npad: int, wcols: int, K: np.ndarray, ld: int, ev: bool = False,
                     bstride: int = 0, device: int = -1):
    """launch_gram_lower_split (test hook gogp_test_gram_split); kp: one kparams(), or a list of k of them (candidates,
    matrix and parameters bstride elements apart).  K: float64 or float32."""
    arr, k = _kp_array(kp)
    X, K = _vec(X, "X"), _mat(K, "K").copy()
    rc = _lib.hooks().gogp_test_gram_split(device, _prec(K), arr, int(ev), _dp(X), X.size, n, npad, wcols, k, bstride,
                                           K.ctypes.data, K.size, ld)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_gram_split")
    return K


def gram_local_check(kp, X: np.ndarray, n: int, npad: int, mrows: int, ncols: int, grid, K: np.ndarray, ld: int,
                     nb_shift: int = 9, ev: bool = False, device: int = -1):
    """launch_gram_local (test hook gogp_test_gram_local); grid = (pr, Pr, pc, Pc)."""
    X, K = _vec(X, "X"), _mat(K, "K").copy()
    pr, Pr, pc, Pc = grid
    rc = _lib.hooks().gogp_test_gram_local(device, _prec(K), ctypes.byref(kp), int(ev), _dp(X), X.size, n, npad, mrows,
                                           ncols, nb_shift, pr, Pr, pc, Pc, K.ctypes.data, K.size, ld)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_gram_local")
    return K


def cross_check(kp, X: np.ndarray, n: int, npad: int, Z: np.ndarray, m: int, mpad: int, KsT: np.ndarray, ld: int,
                ev: bool = False, device: int = -1):
    """launch_cross (test hook gogp_test_cross); KsT: float64 or float32."""
    X, Z, KsT = _vec(X, "X"), _vec(Z, "Z"), _mat(KsT, "KsT").copy()
    rc = _lib.hooks().gogp_test_cross(device, _prec(KsT), ctypes.byref(kp), int(ev), _dp(X), X.size, n, npad, _dp(Z), Z.size,
                                      m, mpad, KsT.ctypes.data, KsT.size, ld)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cross")
    return KsT


def prior_check(kp, Z: np.ndarray, m: int, prior: np.ndarray, device: int = -1):
    """launch_prior (test hook gogp_test_prior)."""
    Z, prior = _vec(Z, "Z"), _vec(prior, "prior").copy()
    rc = _lib.hooks().gogp_test_prior(device, ctypes.byref(kp), _dp(Z), Z.size, m, _dp(prior), prior.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_prior")
    return prior


def kmatvec_check(kp, X: np.ndarray, n: int, npad: int, v: np.ndarray, y, part: np.ndarray, nslab: int, out: np.ndarray,
                  part_idx: int = 0, nparts: int = 1, radial1: bool = False, ev: bool = False, device: int = -1):
    """launch_residual (y given: out = y - K v) or launch_kmatvec_share (y None: the share part_idx of nparts of K v)
    (test hook gogp_test_kmatvec); returns copies of (part, out)."""
    X, v = _vec(X, "X"), _vec(v, "v")
    y = None if y is None else _vec(y, "y")
    part, out = _vec(part, "part").copy(), _vec(out, "out").copy()
    rc = _lib.hooks().gogp_test_kmatvec(device, ctypes.byref(kp), int(radial1), int(ev), _dp(X), X.size, n, npad, _dp(v),
                                        v.size, _dp(y), 0 if y is None else y.size, part_idx, nparts, nslab, _dp(part),
                                        part.size, _dp(out), out.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_kmatvec")
    return part, out


def pgrad_slabs(npad: int, m: int):
    """(slabs, 64-row tiles per slab) of launch_pgrad.  No device."""
    tps = ctypes.c_int(0)
    ns = _lib.hooks().gogp_test_pgrad_slabs(npad, m, ctypes.byref(tps))
    if ns < 0:
        raise GogpError(_lib.GOGP_EARG, "test_pgrad_slabs")
    return int(ns), int(tps.value)


def pgrad_check(kp, X: np.ndarray, n: int, npad: int, Z: np.ndarray, m: int, alpha: np.ndarray, Wt: np.ndarray, ld: int,
                sigma: np.ndarray, part: np.ndarray, dmu: np.ndarray, dsigma: np.ndarray, ev: bool = False,
                device: int = -1):
    """launch_pgrad (test hook gogp_test_pgrad); returns copies of (part, dmu, dsigma)."""
    X, Z, alpha, Wt, sigma = _vec(X, "X"), _vec(Z, "Z"), _vec(alpha, "alpha"), _vec(Wt, "Wt"), _vec(sigma, "sigma")
    part, dmu, dsigma = _vec(part, "part").copy(), _vec(dmu, "dmu").copy(), _vec(dsigma, "dsigma").copy()
    rc = _lib.hooks().gogp_test_pgrad(device, ctypes.byref(kp), int(ev), _dp(X), X.size, n, npad, _dp(Z), Z.size, m,
                                      _dp(alpha), alpha.size, _dp(Wt), Wt.size, ld, _dp(sigma), sigma.size, _dp(part),
                                      part.size, _dp(dmu), dmu.size, _dp(dsigma), dsigma.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_pgrad")
    return part, dmu, dsigma


# ---- the kernels of cg.hip (include/gogp_testhooks.h; tests/test_cg_kernels.py).  Flat host arrays in, copies of the in /
# out arrays back; a refusal or a device error raises GogpError.  The per-column state: sc, float64 of 6 x 64 (rho, a,
# beta, |b|^2, |r|^2, p^T q); st, int32 of 4 x 64 (frozen, iterations, bad, status).
CG_DOT_MODES = {"plain": 0, "bnorm": 1, "rho0": 2, "pq": 3, "rr": 4, "beta": 5}


def _i32(a, what):
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
        raise TypeError("%s: a C-contiguous int32 array" % what)
    return a


def _i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _opt(a, what):
    return (None, 0) if a is None else (_dp(_vec(a, what)), a.size)


def kmm_slabs(rows: int, cols: int) -> int:
    """The slabs of column tiles the product splits rows x cols pairs into.  No device."""
    r = int(_lib.hooks().gogp_test_kmm_slabs(rows, cols))
    if r < 0:
        raise GogpError(_lib.GOGP_EARG, "test_kmm_slabs")
    return r


def cg_dot_blocks(n: int) -> int:
    """The partial sums per column of launch_cg_dots for vectors of n elements.  No device."""
    r = int(_lib.hooks().gogp_test_cg_dot_blocks(n))
    if r < 0:
        raise GogpError(_lib.GOGP_EARG, "test_cg_dot_blocks")
    return r


def kmm_check(kp, A: np.ndarray, rows: int, B, cols: int, V: np.ndarray, ldv: int, T: int, diag, nslab: int,
              part: np.ndarray, Out: np.ndarray, ldo: int, max_blocks: int = 0, device: int = -1):
    """launch_kmm (test hook gogp_test_kmm): B None is the square product on the rows of A, the only form that takes
    diag.  Returns copies of (part, Out)."""
    A, V = _vec(A, "A"), _vec(V, "V")
    part, Out = _vec(part, "part").copy(), _vec(Out, "Out").copy()
    bp, bl = _opt(B, "B")
    dg, dl = _opt(diag, "diag")
    rc = _lib.hooks().gogp_test_kmm(device, ctypes.byref(kp), _dp(A), A.size, rows, bp, bl, cols, _dp(V), V.size, ldv, T,
                                    dg, dl, nslab, max_blocks, _dp(part), part.size, _dp(Out), Out.size, ldo)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_kmm")
    return part, Out


def cg_dots_check(A: np.ndarray, B: np.ndarray, ld: int, n: int, T: int, mode, it: int, tol: float, part: np.ndarray, out,
                  sc: np.ndarray, st: np.ndarray, device: int = -1):
    """launch_cg_dots (test hook gogp_test_cg_dots); mode: a key of CG_DOT_MODES or its number.  Returns copies of
    (part, out, sc, st); out may be None except in mode "plain"."""
    A, B = _vec(A, "A"), _vec(B, "B")
    part, sc, st = _vec(part, "part").copy(), _vec(sc, "sc").copy(), _i32(st, "st").copy()
    out = None if out is None else _vec(out, "out").copy()
    rc = _lib.hooks().gogp_test_cg_dots(device, _dp(A), A.size, _dp(B), B.size, ld, n, T,
                                        CG_DOT_MODES.get(mode, mode), it, float(tol), _dp(part), part.size, _dp(out),
                                        0 if out is None else out.size, _dp(sc), sc.size, _i32p(st), st.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_dots")
    return part, out, sc, st


def cg_update_xr_check(x: np.ndarray, r: np.ndarray, p: np.ndarray, q: np.ndarray, ld: int, n: int, T: int, sc: np.ndarray,
                       st: np.ndarray, device: int = -1):
    """launch_cg_update_xr (test hook gogp_test_cg_update_xr); returns copies of (x, r)."""
    x, r = _vec(x, "x").copy(), _vec(r, "r").copy()
    p, q, sc, st = _vec(p, "p"), _vec(q, "q"), _vec(sc, "sc"), _i32(st, "st")
    rc = _lib.hooks().gogp_test_cg_update_xr(device, _dp(x), x.size, _dp(r), r.size, _dp(p), p.size, _dp(q), q.size, ld, n, T,
                                             _dp(sc), sc.size, _i32p(st), st.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_update_xr")
    return x, r


def cg_update_p_check(p: np.ndarray, z: np.ndarray, ld: int, n: int, T: int, sc: np.ndarray, st: np.ndarray,
                      device: int = -1):
    """launch_cg_update_p (test hook gogp_test_cg_update_p); returns a copy of p."""
    p = _vec(p, "p").copy()
    z, sc, st = _vec(z, "z"), _vec(sc, "sc"), _i32(st, "st")
    rc = _lib.hooks().gogp_test_cg_update_p(device, _dp(p), p.size, _dp(z), z.size, ld, n, T, _dp(sc), sc.size, _i32p(st),
                                            st.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_update_p")
    return p


def cg_scale_check(src: np.ndarray, w, sub, ld: int, n: int, T: int, out: np.ndarray, device: int = -1):
    """launch_cg_scale (test hook gogp_test_cg_scale): out = src o w - sub, w and sub optional; returns a copy of out."""
    src, out = _vec(src, "src"), _vec(out, "out").copy()
    wp, wl = _opt(w, "w")
    sp, sl = _opt(sub, "sub")
    rc = _lib.hooks().gogp_test_cg_scale(device, _dp(src), src.size, wp, wl, sp, sl, ld, n, T, _dp(out), out.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_scale")
    return out


def cg_status_check(T: int, st: np.ndarray, device: int = -1):
    """launch_cg_status (test hook gogp_test_cg_status); returns a copy of st."""
    st = _i32(st, "st").copy()
    rc = _lib.hooks().gogp_test_cg_status(device, T, _i32p(st), st.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_status")
    return st


def cg_precond_check(Ls, ldn: int, n: int, r: int, dis: np.ndarray, Cinv, R: np.ndarray, ld: int, T: int, Z: np.ndarray,
                     C=None, device: int = -1):
    """The preconditioner's application Z = P^-1 R on a given scaled factor (test hook gogp_test_cg_precond); r == 0:
    Jacobi (Ls and Cinv None).  Returns a copy of Z, or of (Z, C) where C is given (it receives I + Ls^T Ls)."""
    dis, R, Z = _vec(dis, "dis"), _vec(R, "R"), _vec(Z, "Z").copy()
    lp, ll = _opt(Ls, "Ls")
    cp, cl = _opt(Cinv, "Cinv")
    C = None if C is None else _vec(C, "C").copy()
    rc = _lib.hooks().gogp_test_cg_precond(device, lp, ll, ldn, n, r, _dp(dis), dis.size, cp, cl, _dp(R), R.size, ld, T,
                                           _dp(Z), Z.size, _dp(C), 0 if C is None else C.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_precond")
    return Z if C is None else (Z, C)


def cg_grad_check(kp, X: np.ndarray, n: int, A: np.ndarray, B: np.ndarray, ld: int, S: int, out: np.ndarray,
                  scale: float = 1.0, accumulate: bool = False, device: int = -1):
    """launch_cg_grad (test hook gogp_test_cg_grad): the slot sums of (scale sum_s A[s][i] B[s][j]) theta dk/dtheta over
    the pairs i, j < n.  Returns a copy of out (NACC slots, extra elements untouched)."""
    X, A, B, out = _vec(X, "X"), _vec(A, "A"), _vec(B, "B"), _vec(out, "out").copy()
    if out.size < NACC:
        raise ValueError("out: NACC slots")
    rc = _lib.hooks().gogp_test_cg_grad(device, ctypes.byref(kp), _dp(X), X.size, n, _dp(A), A.size, _dp(B), B.size, ld, S,
                                        float(scale), int(bool(accumulate)), _dp(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_grad")
    return out


def cg_probes_check(Ls, ldn: int, n: int, r: int, d: np.ndarray, Xi: np.ndarray, ldxi: int, ld: int, T: int, Z: np.ndarray,
                    device: int = -1):
    """launch_cg_probes (test hook gogp_test_cg_probes): Z[t][i] = sqrt(d_i) (sum_k Ls[i][k] Xi[t][n + k] + Xi[t][i]);
    returns a copy of Z."""
    d, Xi, Z = _vec(d, "d"), _vec(Xi, "Xi"), _vec(Z, "Z").copy()
    lp, ll = _opt(Ls, "Ls")
    rc = _lib.hooks().gogp_test_cg_probes(device, lp, ll, ldn, n, r, _dp(d), d.size, _dp(Xi), Xi.size, ldxi, ld, T, _dp(Z),
                                          Z.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_probes")
    return Z


def cg_quadrature(a: np.ndarray, beta: np.ndarray, rho0: float) -> float:
    """rho0 e_1^T log(T) e_1 of the Lanczos tridiagonal of the CG coefficients a, beta (test hook
    gogp_test_cg_quadrature: the host routine of gogp_cg_lml_gradient).  No device."""
    a, beta = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    if a.size != beta.size:
        raise ValueError("a and beta: one entry per iteration each")
    out = np.zeros(1)
    rc = _lib.hooks().gogp_test_cg_quadrature(_dp(a) if a.size else None, _dp(beta) if a.size else None, a.size,
                                              float(rho0), _dp(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_cg_quadrature")
    return float(out[0])


def vecchia_blocks(targets: int, max_blocks: int = 0) -> int:
    """The workgroups (rows of partial sums) of a Vecchia launch over ``targets`` targets.  No device."""
    r = int(_lib.hooks().gogp_test_vecchia_blocks(targets, max_blocks))
    if r < 0:
        raise GogpError(_lib.GOGP_EARG, "test_vecchia_blocks")
    return r


def vecchia_check(kp, X: np.ndarray, y: np.ndarray, v, n: int, nbr, m: int, terms, partials=None, vpart=None, Z=None,
                  targets=None, max_blocks: int = 0, device: int = -1):
    """The kernel of vecchia.hip on caller-supplied parameters, rows, table and y (test hook gogp_test_vecchia).  Observe
    (Z None): terms (n x 3 or None), vpart (one value per workgroup) and, where ``partials`` is given, the workgroups' rows
    of NACC slot sums.  Produce (Z given, ``targets`` rows): terms is targets x 2 (mu, sigma).  nbr: int32, targets x m
    (None with m == 0).  Returns copies: (terms, partials, vpart, value, info) with info = the lowest failing target + 1."""
    X, y = _vec(X, "X"), _vec(y, "y")
    produce = Z is not None
    targets = n if targets is None else targets
    vp, vl = _opt(v, "v")
    zp, zl = _opt(Z, "Z")
    terms = None if terms is None else _vec(terms, "terms").copy()
    partials = None if partials is None else _vec(partials, "partials").copy()
    vpart = None if vpart is None else _vec(vpart, "vpart").copy()
    nb = None if nbr is None else _i32(nbr, "nbr")
    value, info = np.zeros(1), np.zeros(1, dtype=np.int64)
    rc = _lib.hooks().gogp_test_vecchia(
        device, ctypes.byref(kp), int(produce), int(partials is not None), _dp(X), X.size, _dp(y), y.size, vp, vl, n, zp, zl,
        targets, None if nb is None else _i32p(nb), 0 if nb is None else nb.size, m, _dp(terms),
        0 if terms is None else terms.size, _dp(partials), 0 if partials is None else partials.size, _dp(vpart),
        0 if vpart is None else vpart.size, _dp(value), _ip(info), max_blocks)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_vecchia")
    return terms, partials, vpart, float(value[0]), int(info[0])


def vecchia_knn_plan(targets: int, n: int, m: int):
    """(targets of a tile, slabs, bytes of workspace) of a search of ``targets`` targets over n candidates (test hook
    gogp_test_vecchia_knn_plan): tile t holds the targets [t tile, (t + 1) tile), slab s the candidates [s L, (s + 1) L)
    with L = ceil(n / slabs).  No device."""
    out = np.zeros(3, dtype=np.int64)
    rc = _lib.hooks().gogp_test_vecchia_knn_plan(targets, n, m, _ip(out))
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_vecchia_knn_plan")
    return int(out[0]), int(out[1]), int(out[2])


def vecchia_knn_check(X: np.ndarray, n: int, ndim: int, m: int, nbr, d2, xs: np.ndarray, Z=None, targets=None, lengths=None,
                      slabs: int = 0, tile_cap: int = 0, device: int = -1):
    """The search of vecchia_knn.hip on caller-supplied rows (test hook gogp_test_vecchia_knn): the causal table of the n
    rows of X, or (Z given) of ``targets`` rows of Z against them.  nbr (int32) and d2: targets x m at least, xs: n x ndim
    at least; what lies behind comes back as it went in.  Returns copies: (nbr, d2, xs)."""
    X = _vec(X, "X")
    targets = n if targets is None else targets
    zp, zl = _opt(Z, "Z")
    lp = None if lengths is None else _dp(_vec(lengths, "lengths"))
    if lengths is not None and lengths.size != ndim:
        raise GogpError(_lib.GOGP_EARG, "test_vecchia_knn: lengths")
    nb = None if nbr is None else _i32(nbr, "nbr").copy()
    dd = None if d2 is None else _vec(d2, "d2").copy()
    xs = _vec(xs, "xs").copy()
    rc = _lib.hooks().gogp_test_vecchia_knn(device, _dp(X), X.size, n, ndim, zp, zl, targets, lp, m, slabs, tile_cap,
                                            None if nb is None else _i32p(nb), 0 if nb is None else nb.size, _dp(dd),
                                            0 if dd is None else dd.size, _dp(xs), xs.size)
    if rc != _lib.GOGP_OK:
        raise GogpError(rc, "test_vecchia_knn")
    return nb, dd, xs
