"""The Hessian of the LML in the log hyperparameters (gogp_lml_hessian, csrc/hessian.hip) and what it is for: the
Laplace approximation over the hyperparameters (Rasmussen & Williams section 5.2).  No reference counterpart.

    lml_hessian(gp)              the (P, P) Hessian at the parameters of the last Absorb / Observe of ``gp``
    laplace_evidence(gp, x)      covariance and standard errors of log theta^ and the evidence corrected for the width
                                 of the optimum -- host arithmetic on the Hessian
    kmm_check(...)               the tile product K^-1 dK alone (test hook gogp_test_hess_kmm)

Functions of a module, not methods of GP: the handle is the same, the class keeps the reference's surface.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

#: the slot types of a group (csrc/hess_eval.h): the term's value, its length, an ARD length, the period
VALUE, LEN, ARD, PERIOD = 0, 1, 2, 3


def lml_hessian(gp) -> np.ndarray:
    """d2 LML / d log theta_i d log theta_j, (P, P) with the noise parameter last, symmetric bit for bit, at the parameters
    of the last Absorb / Observe / restore of ``gp`` (a gogp_amd.gp.GP).  Works wherever ``gp.LOOGradient`` works and
    leaves the process as it found it.  fp64, unsharded handles without event discounts."""
    P = len(gp.ThetaSimil) + len(gp.ThetaNoise)
    H = np.zeros((P, P))
    gp._check(_lib.lib().gogp_lml_hessian(gp._h, H.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return H


def laplace_evidence(gp, x, log_prior=None) -> dict:
    """The Laplace approximation over the hyperparameters around x = log theta^, a maximum of the LML (plus the log
    prior, whose Hessian in log theta ``log_prior`` (P, P) is then added): observes ``gp`` at x and returns

        lml         the LML at x
        hessian     H, the Hessian of the objective in log theta
        cov         (-H)^-1, the covariance of log theta^
        stderr      the square roots of its diagonal
        evidence    lml + P / 2 log 2 pi - 1/2 log det(-H)

    (the log prior's VALUE is the caller's to add to lml and evidence).  ValueError if -H is not positive definite: x
    is not a maximum."""
    x = np.asarray(x, dtype=float).reshape(-1)
    lml = float(gp.Observe(x))
    return laplace_from_hessian(lml, lml_hessian(gp), log_prior)


def laplace_from_hessian(lml: float, H: np.ndarray, log_prior=None) -> dict:
    H = np.array(H, dtype=float)
    if log_prior is not None:
        H = H + np.asarray(log_prior, dtype=float).reshape(H.shape)
    P = len(H)
    try:
        L = np.linalg.cholesky(-H)
    except np.linalg.LinAlgError:
        raise ValueError("laplace_evidence: -H is not positive definite (x is not a maximum)") from None
    Li = np.linalg.solve(L, np.eye(P))
    cov = Li.T @ Li
    return dict(lml=lml, hessian=H, cov=cov, stderr=np.sqrt(np.diag(cov)),
                evidence=lml + 0.5 * P * np.log(2.0 * np.pi) - float(np.log(np.diag(L)).sum()))


def kmm_check(kp, term: int, types, dims, X: np.ndarray, n: int, npad: int, Kinv: np.ndarray, ld: int, M: np.ndarray,
              device: int = -1) -> np.ndarray:
    """launch_hess_kmm (test hook gogp_test_hess_kmm): M[q] = Kinv @ dK / dlog(slot q) for the slots (types[q], dims[q])
    of term ``term`` of the parameter block kp (gp.kparams).  X: n rows of NDim; Kinv: n rows of ld, read on j <= i only;
    M: len(types) matrices of npad x npad, a copy of which is returned as the launch left it."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1)
    Kinv = np.ascontiguousarray(Kinv, dtype=np.float64).reshape(-1)
    M = np.ascontiguousarray(M, dtype=np.float64).copy()
    ty = np.ascontiguousarray(types, dtype=np.int32)
    dm = np.ascontiguousarray(dims, dtype=np.int32)
    i32, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    rc = _lib.hooks().gogp_test_hess_kmm(device, ctypes.byref(kp), term, ty.size, ty.ctypes.data_as(i32), dm.ctypes.data_as(i32),
                                         X.ctypes.data_as(dp), X.size, n, npad, Kinv.ctypes.data_as(dp), Kinv.size, ld,
                                         M.ctypes.data_as(dp), M.size)
    if rc != _lib.GOGP_OK:
        raise RuntimeError("gogp_test_hess_kmm: error %d" % rc)
    return M
