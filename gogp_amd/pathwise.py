"""Pathwise posterior samples (gogp_pathwise_*, csrc/pathwise.hip): posterior FUNCTION draws by Matheron's rule (Wilson et
al. 2020, "Efficiently sampling functions from Gaussian process posteriors").  No reference counterpart.

    f_s(z) = phi(z)^T w_s + k(z, X) v_s,      v_s = K^^-1 (y - Phi(X) w_s - eps_s)

    spectral_features(gp, R)     R random Fourier features of the prior at the handle's current parameters
    draw(gp, S, R)               S draws, fixed once: a Paths
    Paths(Z), Paths.gradient(Z)  their values (S, m) and derivatives in z (S, m, NDim) at any number of points
    features_check, crossgrad_check   the two kernels alone (test hooks)

Functions of a module, not methods of GP (as gogp_amd.hessian).  A Paths owns copies of everything it reads: it stays valid
and keeps its bits whatever happens to the GP afterwards.  All randomness is drawn here, on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .kernel import K_MATERN32, K_MATERN52, K_MATERN52_TEXTBOOK, K_NORMAL, K_PERIODIC

_DP = ctypes.POINTER(ctypes.c_double)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(_DP)


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def spectral_features(gp, R: int, normals=None, rng=None):
    """(Omega (R, NDim), phase (R), amp (R)) with sum_r phi_r(x) phi_r(x') ~ k(x, x') at gp.ThetaSimil, phi_r(x) = amp[r]
    cos(Omega[r] . x + phase[r]): draws from the spectral measure of every term --

        Normal                          omega = g / l
        Matern-3/2, textbook Matern-5/2 omega = g / (l sqrt(u / 2 nu)),  u ~ chi^2(2 nu)   (a multivariate t)

    with g ~ N(0, I) (``normals`` (R, NDim) when given), l per dimension for an ARD term, phase ~ U[0, 2 pi).  A Scaled
    term or a Sum gives every term t a block of R_t features (R split evenly, the first terms one more) with amp =
    sqrt(2 c_t / R_t).  ValueError for a Periodic term (a line spectrum: not implemented) and for the reference's Matern52,
    whose r^2 coefficient is 1, not 5/3: it is not a Matern kernel and has no known spectral measure."""
    rng = np.random.default_rng() if rng is None else rng
    D, terms, theta = gp.NDim, gp.Simil.terms, np.asarray(gp.ThetaSimil, dtype=float)
    R = int(R)
    if R < len(terms):
        raise ValueError("spectral_features: at least one feature per term")
    for t in terms:
        if t.kind == K_PERIODIC:
            raise ValueError("spectral_features: the Periodic kernel is not supported (bring your own features)")
        if t.kind == K_MATERN52:
            raise ValueError("spectral_features: the reference's Matern52 (coefficient 1, not 5/3) is not a Matern kernel "
                             "and has no known spectral measure; use Matern52Textbook")
    g = rng.standard_normal((R, D)) if normals is None else _f64(normals, (R, D))
    Omega, amp = np.empty((R, D)), np.empty(R)
    r0 = 0
    for i, t in enumerate(terms):
        Rt = R // len(terms) + (1 if i < R % len(terms) else 0)
        length = theta[t.len_idx:t.len_idx + D] if t.ard else np.full(D, theta[t.len_idx])
        c = theta[t.scale_idx] if t.scale_idx >= 0 else 1.0
        w = g[r0:r0 + Rt] / length
        if t.kind != K_NORMAL:
            nu2 = {K_MATERN32: 3, K_MATERN52_TEXTBOOK: 5}[t.kind]
            w = w / np.sqrt(rng.chisquare(nu2, size=(Rt, 1)) / nu2)
        Omega[r0:r0 + Rt], amp[r0:r0 + Rt] = w, np.sqrt(2.0 * c / Rt)
        r0 += Rt
    return Omega, rng.uniform(0.0, 2.0 * np.pi, size=R), amp


class Paths:
    """S posterior function draws (gogp_paths).  ``paths(Z)``: (S, m); ``paths.gradient(Z)``: ((S, m), (S, m, NDim));
    ``paths.V``: (S, n), the weights of k(., X).  Close it (or use it as a context manager) to free the device memory."""

    def __init__(self, handle, S: int, n: int, ndim: int):
        self._p, self.S, self.n, self.NDim = handle, int(S), int(n), int(ndim)

    def _eval(self, Z, grad: bool):
        if not self._p:
            raise ValueError("Paths: closed")
        Z = _f64(Z).reshape(-1, self.NDim)
        m = len(Z)
        F = np.zeros((self.S, m))
        dF = np.zeros((self.S, m, self.NDim)) if grad else None
        if m:
            rc = _lib.lib().gogp_pathwise_eval(self._p, _dp(Z), m, _dp(F), _dp(dF) if grad else None)
            if rc != _lib.GOGP_OK:
                from .gp import GogpError
                raise GogpError(rc, "pathwise_eval: error %d" % rc)
        return F, dF

    def __call__(self, Z) -> np.ndarray:
        return self._eval(Z, False)[0]

    def gradient(self, Z):
        return self._eval(Z, True)

    @property
    def V(self) -> np.ndarray:
        if not self._p:
            raise ValueError("Paths: closed")
        V = np.zeros((self.S, self.n))
        rc = _lib.lib().gogp_pathwise_get_v(self._p, _dp(V))
        if rc != _lib.GOGP_OK:
            from .gp import GogpError
            raise GogpError(rc, "pathwise_get_v: error %d" % rc)
        return V

    def close(self):
        if getattr(self, "_p", None):
            _lib.lib().gogp_pathwise_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def draw(gp, S: int, R: int = 1024, rng=None, features=None, W=None, Xi=None) -> Paths:
    """S pathwise draws from the posterior of ``gp`` (a gogp_amd.gp.GP) at the parameters and data of its last Absorb /
    Observe / Append / Remove / restore.  ``features``: (Omega, phase, amp), default spectral_features(gp, R, rng=rng);
    ``W`` (R, S) and ``Xi`` (S, n): the standard normals of the prior draws and of the noise, drawn from ``rng`` when None.
    fp64, unsharded handles without event discounts; the GP is left as found."""
    rng = np.random.default_rng() if rng is None else rng
    Omega, phase, amp = spectral_features(gp, R, rng=rng) if features is None else features
    D, n, S = gp.NDim, len(gp.Y), int(S)
    Omega, phase, amp = _f64(Omega).reshape(-1, D), _f64(phase).reshape(-1), _f64(amp).reshape(-1)
    R = len(amp)
    if len(Omega) != R or len(phase) != R:
        raise ValueError("draw: Omega (R, NDim), phase (R) and amp (R) disagree")
    W = rng.standard_normal((R, max(S, 0))) if W is None else _f64(W)
    Xi = rng.standard_normal((max(S, 0), n)) if Xi is None else _f64(Xi)
    if W.shape != (R, S) or Xi.shape != (S, n):
        raise ValueError("draw: W must be (R, S) and Xi (S, n)")
    p = ctypes.c_void_p()
    gp._check(_lib.lib().gogp_pathwise_create(gp._h, R, _dp(Omega), _dp(phase), _dp(amp), S, _dp(W), _dp(Xi),
                                              ctypes.byref(p)))
    return Paths(p, S, n, D)


def features_check(Omega, phase, amp, Z, W, grad: bool = False, device: int = -1) -> np.ndarray:
    """The feature product alone (test hook gogp_test_pw_features): (S, m), or its derivative in z (S, m, NDim)."""
    Omega, Z, W = _f64(Omega), _f64(Z), _f64(W)
    (R, D), m, S = Omega.shape, len(Z), W.shape[1]
    phase, amp = _f64(phase, (R,)), _f64(amp, (R,))
    out = np.zeros((S, m, D) if grad else (S, m))
    rc = _lib.hooks().gogp_test_pw_features(device, D, R, _dp(Omega), Omega.size, _dp(phase), _dp(amp), _dp(Z), Z.size, m,
                                            _dp(W), W.size, S, int(grad), _dp(out), out.size)
    if rc != _lib.GOGP_OK:
        raise RuntimeError("gogp_test_pw_features: error %d" % rc)
    return out


def crossgrad_check(kp, Z, X, V, device: int = -1) -> np.ndarray:
    """The cross-gradient kernel alone (test hook gogp_test_pw_crossgrad): out[s, i, d] = sum_j dk(z_i, x_j)/dz_d V[s, j]
    for the parameter block kp (gp.kparams)."""
    Z, X, V = _f64(Z), _f64(X), _f64(V)
    (m, D), n, S = Z.shape, len(X), len(V)
    out = np.zeros((S, m, D))
    rc = _lib.hooks().gogp_test_pw_crossgrad(device, ctypes.byref(kp), _dp(Z), Z.size, m, _dp(X), X.size, n, _dp(V), V.size,
                                             V.shape[1], S, _dp(out), out.size)
    if rc != _lib.GOGP_OK:
        raise RuntimeError("gogp_test_pw_crossgrad: error %d" % rc)
    return out
