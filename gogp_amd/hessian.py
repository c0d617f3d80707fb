"""The Hessian of the LML in the log hyperparameters (gogp_lml_hessian, csrc/hessian.hip) and what it is for: the
Laplace approximation over the hyperparameters (Rasmussen & Williams section 5.2).  No reference counterpart.

    lml_hessian(gp)              the (P, P) Hessian at the parameters of the last Absorb / Observe of ``gp``
    laplace_evidence(gp, x)      covariance and standard errors of log theta^ and the evidence corrected for the width
                                 of the optimum -- host arithmetic on the Hessian
    kmm_check(...)               the tile product K^-1 dK alone (test hook gogp_test_hess_kmm)
    pair_check, kvec_check, matvec_check, dots_check, traces_check, quad_check
                                 the other kernels alone (test hooks gogp_test_hess_*)

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


# ---- the other kernels of csrc/hessian.hip alone (tests/test_hessian_kernels.py).  Every wrapper copies its in / out arrays,
# hands every array over whole with its length in elements and returns the copies as the launch left them.
_I32P, _DP = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)


def _f(a, copy=False):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    return a.copy() if copy else a


def _group(types, dims):
    ty, dm = np.ascontiguousarray(types, dtype=np.int32), np.ascontiguousarray(dims, dtype=np.int32)
    return ty, dm, (ty.size, ty.ctypes.data_as(_I32P), dm.ctypes.data_as(_I32P))


def _hook(name, *args):
    rc = getattr(_lib.hooks(), name)(*args)
    if rc != _lib.GOGP_OK:
        raise RuntimeError("%s: error %d" % (name, rc))


def _a(a):
    return (a.ctypes.data_as(_DP), a.size)


def pair_check(kp, term: int, types_a, dims_a, types_b, dims_b, X, alpha, n: int, npad: int, Kinv, ld: int, part, out,
               device: int = -1):
    """launch_hess_pair (gogp_test_hess_pair): the HESS_NMOM second-derivative sums of the groups a and b of term ``term``
    (csrc/hess_eval.h: hess_moments).  Returns (part, out): the lower 64-tiles' sums, rows of 25, and their totals."""
    X, alpha, Kinv, part, out = _f(X), _f(alpha), _f(Kinv), _f(part, True), _f(out, True)
    ka, kb = _group(types_a, dims_a), _group(types_b, dims_b)
    _hook("gogp_test_hess_pair", device, ctypes.byref(kp), term, *ka[2], *kb[2], *_a(X), *_a(alpha), n, npad, *_a(Kinv), ld,
          *_a(part), *_a(out))
    return part, out


def kvec_check(kp, term: int, types, dims, X, alpha, n: int, npad: int, b, ldb: int, device: int = -1) -> np.ndarray:
    """launch_hess_kvec (gogp_test_hess_kvec): b[q] = dK / dlog(slot q) @ alpha; b: len(types) rows of ldb, returned flat."""
    X, alpha, b = _f(X), _f(alpha), _f(b, True)
    g = _group(types, dims)
    _hook("gogp_test_hess_kvec", device, ctypes.byref(kp), term, *g[2], *_a(X), *_a(alpha), n, npad, *_a(b), ldb)
    return b


def matvec_check(M, alpha, n: int, npad: int, S: int, c, device: int = -1) -> np.ndarray:
    """launch_hess_matvec (gogp_test_hess_matvec): c[s] = M[s] @ alpha on the leading n x n; M: S matrices of npad x npad,
    c: S rows of npad, returned flat."""
    M, alpha, c = _f(M), _f(alpha), _f(c, True)
    _hook("gogp_test_hess_matvec", device, *_a(M), *_a(alpha), n, npad, S, *_a(c))
    return c


def dots_check(b, c, alpha, ldv: int, n: int, S: int, dots, device: int = -1) -> np.ndarray:
    """launch_hess_dots (gogp_test_hess_dots): dots[s][t] = b_s . c_t (s <= t < S, zero below), dots[s][S] = alpha . c_s;
    S rows of S + 1, returned flat."""
    b, c, alpha, dots = _f(b), _f(c), _f(alpha), _f(dots, True)
    _hook("gogp_test_hess_dots", device, *_a(b), *_a(c), *_a(alpha), ldv, n, S, *_a(dots))
    return dots


def traces_check(M, S: int, Kinv, ld: int, n: int, npad: int, pairs, part, out, device: int = -1):
    """launch_hess_traces (gogp_test_hess_traces): out[p] = tr(A B), B = M[pairs[p][1]], A = M[pairs[p][0]] or (-1) the
    symmetric Kinv from its stored half.  Returns (part, out)."""
    M, Kinv, part, out = _f(M), _f(Kinv), _f(part, True), _f(out, True)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
    _hook("gogp_test_hess_traces", device, *_a(M), S, *_a(Kinv), ld, n, npad, pr.ctypes.data_as(_I32P), pr.size, *_a(part),
          *_a(out))
    return part, out


def quad_check(Kinv, ld: int, alpha, n: int, npad: int, part, out, device: int = -1):
    """launch_hess_quad (gogp_test_hess_quad): out = alpha^T Kinv alpha, |Kinv|_F^2, |alpha|^2, tr Kinv.  Returns (part, out)."""
    Kinv, alpha, part, out = _f(Kinv), _f(alpha), _f(part, True), _f(out, True)
    _hook("gogp_test_hess_quad", device, *_a(Kinv), ld, *_a(alpha), n, npad, *_a(part), *_a(out))
    return part, out
