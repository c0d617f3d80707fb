"""The tutorial's forecast harness over the HIP path ("next" row 2 of SURVEY.md 8f).

Mirror of tutorial/tutorial.go: ``Evaluate`` (:56-230) -- load a CSV, standardise the
outputs, and for every time point fit the hyperparameters on the points before it and
forecast it one step out of sample -- and ``load`` (:234-272).  Same knobs (module
variables, the reference's package variables :21-33), same output columns, same number
formatting (``%f``), so the case studies of the tutorial run unchanged on a
gogp_amd.gp.GP / gp.Model.

Differences, all forced by what is absent here: the optimiser is gogp_amd.optimize.lbfgs /
Adam instead of gonum's ``optimize.Minimize`` / infergo's ``infer.Adam`` (sources not in the
container: iterate-by-iterate parity unpinned), and the random jitter of the starting
point (:119-121, seeded from the wall clock at :36) takes a ``SEED`` so that runs can be
repeated; SEED = None seeds from the clock as the reference does.
"""
from __future__ import annotations

import csv
import math
import sys
import time
from typing import Optional

import numpy as np

from . import optimize

# package variables of tutorial/tutorial.go:21-33
OPTINP = False
MINOPT = 0
ALG = "lbfgs"
PARALLEL = False
ITERS = 1000       # major iterations
MINITERS = 10      # minimum iterations to accept in lbfgs
THRESHOLD = 1e-6   # gradient threshold
RATE = 0.01        # learning rate (for Adam)
NTASKS = 0
NONORMALIZE = False
OUTOFSAMPLE = False
SEED: Optional[int] = None  # not in the reference: fixes the starting-point jitter
#: not in the reference either: evaluate the windows of N <= GOGP_BATCH_MAX_N rows as batches of small GPs
#: (GP.set_batch / batch_observe_gradient / batch_produce: one launch per round of all windows' L-BFGS runs, which
#: go in lock-step, optimize.lbfgs_lockstep).  Applies with ALG = "lbfgs", OPTINP off, ``m`` the GP itself or a
#: gp.Model around it, and a GP with those methods; otherwise it changes nothing.  Same starting points (the
#: jitter is drawn in window order), same rows in the same order and format, and ``gp`` is left where the
#: sequential harness leaves it (the last window's data, observed at its final x).
#: With OPTINP on, the windows carry their inputs and outputs in x and go through the full-form batch
#: (GP.batch_observe_full_gradient / batch_produce_full).  ``m`` is then the GP itself or a model with a
#: ``window_objective()`` method (priors.AnyNoiseModel, priors.WarpedTimeModel): a fresh host-side object per window
#: that adds the priors -- which memoise at the window's start vector -- and applies the model's edit of the
#: gradient.  A model without it runs the sequential loop.
BATCH = False
BATCH_MAX_N = 128  # include/gogp_hip.h: GOGP_BATCH_MAX_N


def _f(v: float) -> str:
    """Go's fmt %f."""
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "+Inf" if v > 0 else "-Inf"
    return "%f" % v


def load(rdr):
    """tutorial/tutorial.go:234-272: every record is D inputs followed by one output.
    Returns (X as an (n, D) array, y); raises ValueError on a field that is not a number
    (the reference returns the strconv error)."""
    X, y = [], []
    for record in csv.reader(rdr):
        if not record:
            continue
        row = [float(f) for f in record]  # ValueError = the reference's data error
        X.append(row[:-1])
        y.append(row[-1])
    ndim = len(X[0]) if X else 0
    return np.array(X, dtype=float).reshape(len(X), ndim), np.array(y, dtype=float)


def Evaluate(gp, m, theta, rdr, wtr, log=sys.stderr) -> None:
    """tutorial/tutorial.go:56-230.  ``gp``: a GP (NDim, X, Y, Produce); ``m``: the model that is
    optimised (the GP itself or a gp.Model around it); ``theta``: initial LOG hyperparameters;
    ``rdr`` / ``wtr``: text streams of the CSV data and of the forecasts."""
    gp.Parallel = bool(PARALLEL)
    rng = np.random.default_rng(time.time_ns() if SEED is None else SEED)
    theta = np.asarray(theta, dtype=float)

    print("loading...", end="", file=log)
    X, Y = load(rdr)
    print("done", file=log)

    # Normalize Y (gonum stat.MeanStdDev: the unbiased, n-1, standard deviation)
    if NONORMALIZE:
        meany, stdy = 0.0, 1.0
    else:
        meany = float(Y.mean()) if len(Y) else 0.0
        stdy = float(Y.std(ddof=1)) if len(Y) > 1 else float("nan")
        Y = (Y - meany) / stdy

    print("Forecasting...", file=log)
    priors = _batch_priors(gp, m)
    if priors is not None:
        _forecast_batched(gp, m, priors[0], theta, X, Y, meany, stdy, rng, wtr, log, full=OPTINP)
    else:
        for end in range(len(X)):
            # Randomize the initial values of hyperparameters (:119-121)
            jitter = 0.1 * rng.standard_normal(len(theta))
            _forecast_window(gp, m, theta, X, Y, end, jitter, meany, stdy, wtr, log)

    if OUTOFSAMPLE and len(X):
        Z = (X + X[-1])[1:]  # :200-208
        try:
            mu, sigma = gp.Produce(Z)
        except Exception as e:
            print("Failed to forecast: %s" % e, file=log)
            mu = sigma = np.full(len(Z), float("nan"))
        for i in range(len(Z)):
            fields = [_f(v) for v in Z[i]] + ["nan", _f(mu[i] * stdy + meany), _f(sigma[i] * stdy)]
            wtr.write(",".join(fields) + "\n")

    print("done", file=log)


def _write_row(wtr, z, y, mu, sigma, lml0, lml, x, ntheta, meany, stdy) -> None:
    fields = [_f(v) for v in z]
    fields += [_f(y * stdy + meany), _f(mu * stdy + meany), _f(sigma * stdy), _f(lml0), _f(lml)]
    fields += [_f(math.exp(v)) for v in x[:ntheta]]
    wtr.write(",".join(fields) + "\n")


def _forecast_window(gp, m, theta, X, Y, end, jitter, meany, stdy, wtr, log) -> None:
    """One window of tutorial/tutorial.go:88-197: fit on the points before ``end``, forecast point ``end``."""
    Xi, Yi = X[:end], Y[:end]
    if OPTINP:
        # inputs and outputs ride in the parameter vector of Observe (:100-110)
        x = np.concatenate([theta, Xi.reshape(-1), Yi])
    else:
        x = theta.copy()
        gp.X, gp.Y = Xi, Yi
    x[:len(theta)] += jitter

    lml0 = m.Observe(x)  # Initial log likelihood

    if len(gp.X) > MINOPT:
        if ALG == "lbfgs":
            try:
                # optimize.Settings.Concurrent = NTASKS (tutorial.go:141): evaluate that many trial
                # points per round -- here the line search's next NTASKS steps in one launch
                # sequence (hyperparameters-only form on a GP / gp.Model with the candidates call)
                conc = NTASKS if (NTASKS > 1 and not OPTINP and
                                  hasattr(getattr(m, "GP", m), "observe_gradient_candidates")) else 1
                result = optimize.lbfgs(m, x, major_iterations=ITERS, gradient_threshold=THRESHOLD,
                                        line_search_candidates=conc)
                if not result.converged and result.iterations <= MINITERS:
                    print("%d: stuck after %d iterations" % (end, result.iterations), file=log)
                x = result.x
            except ValueError as e:  # infeasible start
                print("%d: stuck after 0 iterations: %s" % (end, e), file=log)
        elif ALG == "adam":
            opt = optimize.Adam(Rate=RATE)
            for _ in range(ITERS):
                _, grad = opt.Step(m, x)
                if not (np.abs(grad) >= THRESHOLD).any():
                    break
        else:
            raise ValueError("ALG must be lbfgs or adam")

    lml = m.Observe(x)  # Final log likelihood

    Z = X[end:end + 1]
    try:
        mu, sigma = gp.Produce(Z)
    except Exception as e:  # the reference prints and carries on (:179-181)
        print("Failed to forecast: %s" % e, file=log)
        mu, sigma = [float("nan")], [float("nan")]
    _write_row(wtr, Z[0], Y[end], mu[0], sigma[0], lml0, lml, x, len(theta), meany, stdy)


def _batch_priors(gp, m):
    """(priors,) when BATCH applies (priors None: ``m`` is the GP itself), else None.  With OPTINP: (factory,), the
    model's ``window_objective`` (None: ``m`` is the GP itself)."""
    if not (BATCH and ALG == "lbfgs"):
        return None
    if OPTINP:
        if not all(hasattr(gp, a) for a in ("batch_observe_full_gradient", "batch_produce_full")):
            return None
        if m is gp:
            return (None,)
        if getattr(m, "GP", None) is gp and callable(getattr(m, "window_objective", None)):
            return (m.window_objective,)
        return None
    if not all(hasattr(gp, a) for a in ("set_batch", "batch_observe_gradient", "batch_produce")):
        return None
    if m is gp:
        return (None,)
    if getattr(m, "GP", None) is gp and hasattr(m, "Priors"):
        return (m.Priors,)
    return None


def _forecast_batched(gp, m, priors, theta, X, Y, meany, stdy, rng, wtr, log, full=False) -> None:
    """The windows of _forecast_window as batches of small GPs (BATCH): every window's starting point first (the
    jitter in window order: the starts of the sequential harness), the initial LML of every window in one call,
    the L-BFGS runs of the windows in lock-step (one call per round), then the final LML and the one-point forecast
    of every window in one call.  Windows of more than BATCH_MAX_N rows, and a window whose initial LML cannot be
    formed (the sequential harness raises there), take the sequential code at their turn.
    ``full`` (OPTINP): every window carries its inputs and outputs in x (:100-110), the vectors differ in length and go
    through the full-form batch; ``priors`` is then the model's window_objective, called once per window."""
    ntheta = len(theta)
    jitters, starts = [], []
    for end in range(len(X)):
        jitters.append(0.1 * rng.standard_normal(ntheta))  # (:119-121)
        x = np.concatenate([theta, X[:end].reshape(-1), Y[:end]]) if full else theta.copy()
        x[:ntheta] += jitters[-1]
        starts.append(x)
    wins = [end for end in range(len(X)) if end <= BATCH_MAX_N]  # window end holds n = end rows
    member = {end: i for i, end in enumerate(wins)}
    objective = {e: priors() for e in wins} if full and priors is not None else {}

    def model_value(x, lml, grad, e=None):  # gp/model.go:17-28, as gp.Model adds the priors
        if priors is None:
            return lml, grad
        if full:  # ... and as the model around it edits the gradient
            return objective[e].value_grad(x, lml, grad)
        v = lml + priors.Observe(x)
        pg = np.asarray(priors.Gradient(), dtype=float)
        g = np.array(grad, dtype=float)
        g[:len(pg)] += pg
        return v, g

    def observe_gradient(xs, ends):
        if full:
            return gp.batch_observe_full_gradient(list(xs))
        return gp.batch_observe_gradient(xs, members=[member[e] for e in ends])

    done = {}  # end -> (lml0, x, lml, mu, sigma, note)
    if wins:
        if full:
            l0, g0, s0 = observe_gradient([starts[e] for e in wins], wins)
        else:
            gp.set_batch(X, Y, [(0, end) for end in wins])
            l0, g0, s0 = gp.batch_observe_gradient(np.array([starts[e] for e in wins]))
        lml0 = {e: model_value(starts[e], float(l0[i]), g0[i], e)[0] for i, e in enumerate(wins) if s0[i] == 0}
        runs = [e for e in wins if e in lml0 and e > MINOPT]

        def evaluate(idx, xs):
            lm, gr, st = observe_gradient(xs, [runs[i] for i in idx])
            out = []
            for j in range(len(xs)):
                if st[j] != 0 or not np.isfinite(lm[j]):
                    out.append((np.inf, None))
                    continue
                v, g = model_value(xs[j], float(lm[j]), gr[j], runs[idx[j]])
                out.append((-v, -g) if np.isfinite(v) else (np.inf, None))
            return out

        results = optimize.lbfgs_lockstep(evaluate, [starts[e] for e in runs], major_iterations=ITERS,
                                          gradient_threshold=THRESHOLD) if runs else []
        xfin, notes = {e: starts[e] for e in lml0}, {}
        for e, r in zip(runs, results):
            if r is None:
                notes[e] = "%d: stuck after 0 iterations: %s" % (e, optimize.INFEASIBLE_START)
                continue
            if not r.converged and r.iterations <= MINITERS:
                notes[e] = "%d: stuck after %d iterations" % (e, r.iterations)
            xfin[e] = r.x
        fin = sorted(lml0)
        if fin:
            if full:
                lf, mus, sigmas, sf = gp.batch_produce_full([xfin[e] for e in fin], [X[e:e + 1] for e in fin])
            else:
                lf, mus, sigmas, sf = gp.batch_produce(np.array([xfin[e] for e in fin]), [X[e:e + 1] for e in fin],
                                                       members=[member[e] for e in fin])
            for i, e in enumerate(fin):
                if priors is None:
                    lml = float(lf[i])
                elif full:
                    lml = objective[e].value(xfin[e], float(lf[i]))
                else:
                    lml = float(lf[i]) + priors.Observe(xfin[e])
                mu, sigma = mus[i][0], sigmas[i][0]
                if sf[i] != 0:
                    mu = sigma = float("nan")
                done[e] = (lml0[e], xfin[e], lml, mu, sigma, notes.get(e), sf[i])

    for end in range(len(X)):
        if end not in done:
            _forecast_window(gp, m, theta, X, Y, end, jitters[end], meany, stdy, wtr, log)
            continue
        l0, x, lml, mu, sigma, note, status = done[end]
        if note:
            print(note, file=log)
        if status != 0:
            print("Failed to forecast: status %d" % status, file=log)
        _write_row(wtr, X[end], Y[end], mu, sigma, l0, lml, x, ntheta, meany, stdy)
    # the GP as the sequential harness leaves it: the last window's data, observed at its final x
    last = len(X) - 1
    if last in done:
        if not full:  # (full: Observe re-slices X and Y out of x)
            gp.X, gp.Y = X[:last], Y[:last]
        if done[last][6] == 0:
            m.Observe(done[last][1])
