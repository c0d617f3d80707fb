"""Host-side builders of basis-function matrices for GP.SetBasis / GP.BasisProduce.

Each returns H, one row per input point and one column per basis function; the caller evaluates the same builder with
the same arguments at the test points for GP.BasisProduce.  ``polynomial`` centres and scales the coordinates, so pass
the ``center`` and ``scale`` it should use at the test points (by default they are taken from the points given, which
differ between training and test inputs): ``polynomial_frame(X)`` returns the pair for the training inputs.
"""
import numpy as np


def _points(X) -> np.ndarray:
    x = np.asarray(X, dtype=float)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.ndim != 2:
        raise ValueError("X must be n x D")
    return x


def polynomial_frame(X, axes=None):
    """(center, scale) of the chosen coordinates of X: the midpoint and the half-range (1 where a coordinate is
    constant), so that the scaled coordinates lie in [-1, 1]."""
    x = _points(X)
    ax = list(range(x.shape[1])) if axes is None else [int(a) for a in axes]
    sel = x[:, ax]
    if len(sel) == 0:
        return np.zeros(len(ax)), np.ones(len(ax))
    lo, hi = sel.min(axis=0), sel.max(axis=0)
    half = 0.5 * (hi - lo)
    return 0.5 * (hi + lo), np.where(half > 0.0, half, 1.0)


def polynomial(X, degree: int, axes=None, center=None, scale=None) -> np.ndarray:
    """The constant and the powers 1 .. degree of each chosen coordinate (no cross terms): 1 + degree * len(axes)
    columns, the coordinates shifted by ``center`` and divided by ``scale`` (default: polynomial_frame(X, axes)) so that
    the columns stay of order one."""
    x = _points(X)
    if degree < 0:
        raise ValueError("degree must be >= 0")
    ax = list(range(x.shape[1])) if axes is None else [int(a) for a in axes]
    for a in ax:
        if a < 0 or a >= x.shape[1]:
            raise ValueError("axis %d out of range" % a)
    c0, s0 = polynomial_frame(x, ax)
    c = c0 if center is None else np.broadcast_to(np.asarray(center, dtype=float), (len(ax),))
    s = s0 if scale is None else np.broadcast_to(np.asarray(scale, dtype=float), (len(ax),))
    if np.any(s == 0.0) or not (np.all(np.isfinite(c)) and np.all(np.isfinite(s))):
        raise ValueError("center and scale must be finite, scale non-zero")
    t = (x[:, ax] - c) / s
    cols = [np.ones(len(x))]
    for k in range(len(ax)):
        for d in range(1, degree + 1):
            cols.append(t[:, k] ** d)
    return np.stack(cols, axis=1)


def fourier(X, period: float, harmonics: int, axis: int = 0) -> np.ndarray:
    """sin and cos of 2 pi k x[axis] / period for k = 1 .. harmonics: 2 * harmonics columns, (sin, cos) pairs."""
    x = _points(X)
    if not (period > 0.0) or not np.isfinite(period):
        raise ValueError("period must be positive and finite")
    if harmonics < 1:
        raise ValueError("harmonics must be >= 1")
    if axis < 0 or axis >= x.shape[1]:
        raise ValueError("axis %d out of range" % axis)
    w = 2.0 * np.pi * x[:, axis] / period
    cols = []
    for k in range(1, harmonics + 1):
        cols += [np.sin(k * w), np.cos(k * w)]
    return np.stack(cols, axis=1)


def stack(*parts) -> np.ndarray:
    """The columns of the parts side by side; a constant column (all ones) is kept only the first time it occurs."""
    if not parts:
        raise ValueError("stack: nothing to stack")
    mats = [np.asarray(p, dtype=float) for p in parts]
    mats = [m.reshape(-1, 1) if m.ndim == 1 else m for m in mats]
    n = mats[0].shape[0]
    cols, have_const = [], False
    for m in mats:
        if m.ndim != 2 or m.shape[0] != n:
            raise ValueError("stack: the parts must have the same number of rows")
        for j in range(m.shape[1]):
            const = n > 0 and bool(np.all(m[:, j] == 1.0))
            if const and have_const:
                continue
            have_const = have_const or const
            cols.append(m[:, j])
    return np.stack(cols, axis=1) if cols else np.zeros((n, 0))


def transposed_padded(H, npad: int) -> np.ndarray:
    """H^T as the library stores it: p rows of npad doubles, zero from column n on."""
    h = np.asarray(H, dtype=float)
    n, p = h.shape
    if npad < n:
        raise ValueError("npad < n")
    out = np.zeros((p, npad))
    out[:, :n] = h.T
    return out
