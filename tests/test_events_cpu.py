"""Event discounts on the host (no GPU): kernel.Events' Observe against the walk of tutorial/events/kernel/kernel.go:14-44,
parse_events on the selfcheck flag, gogp_events_check's refusals, and the numpy restatement (tests/events_ref.py)
against a central finite difference of its own LML."""
import math

import numpy as np
import pytest

import events_ref as R
from gogp_amd import kernel

SIMIL = kernel.Scaled(kernel.Matern52)


def _ref_observe(events, c, l, xa, xb):
    r = abs(xa - xb) / l
    k = c * (1.0 + R.S5 * r + r * r) * math.exp(-R.S5 * r)
    return k * R.discount_pair(events, xa, xb)


EV = [(1.0, 1.0, 0.5), (2.0, 3.0, 0.25), (2.5, 4.0, 0.75), (6.0, 7.0, 0.125)]


@pytest.mark.parametrize("xa,xb,disc", [
    (0.5, 1.5, 0.5),    # spans from == to == 1.0
    (1.5, 0.5, 0.5),    # swapped order
    (1.0, 1.0, 1.0),    # equal points: never discounted
    (0.5, 1.0, 0.5),    # exactly on from (== to): from <= xb
    (1.0, 1.5, 1.0),    # starts on the boundary: xa < from fails
    (2.2, 3.0, 0.25),   # exactly on to: to <= xb
    (3.0, 3.5, 1.0),    # starts on event 1's to (xa < to fails) and inside event 2: no boundary between
    (2.7, 3.5, 0.25),   # inside the overlap of events 1 and 2: event 1's to lies between, the first in the list wins
    (2.7, 3.2, 0.25),
    (0.0, 8.0, 0.5),    # spans every event: the first applies
    (4.5, 5.5, 1.0),    # between events
    (6.5, 6.9, 1.0),    # inside event 3, no boundary between
])
def test_events_observe_matches_the_reference_walk(xa, xb, disc):
    k = kernel.Events(SIMIL, EV)
    c, l = 1.7, 0.9
    assert k.NTheta() == SIMIL.NTheta() == 2
    got = k.Observe([c, l, xa, xb])
    want = _ref_observe(EV, c, l, xa, xb)
    assert got == pytest.approx(want, rel=1e-15, abs=0)
    assert R.discount_pair(EV, xa, xb) == disc
    base = SIMIL.Observe([c, l, xa, xb])
    assert got == pytest.approx(base * disc, rel=1e-15)


def test_events_overlapping_first_in_list_wins():
    ev = [(2.0, 5.0, 0.5), (3.0, 4.0, 0.1)]
    k = kernel.Events(SIMIL, ev)
    # (3.5, 4.5): event 0 has no boundary between (2 < 3.5, 5 > 4.5), event 1's to = 4 is: 0.1
    assert k.Observe([1.0, 1.0, 3.5, 4.5]) == pytest.approx(0.1 * SIMIL.Observe([1.0, 1.0, 3.5, 4.5]))
    # (2.5, 4.5): event 0 has none, event 1 has both: 0.1 once (the walk stops)
    assert k.Observe([1.0, 1.0, 2.5, 4.5]) == pytest.approx(0.1 * SIMIL.Observe([1.0, 1.0, 2.5, 4.5]))
    # (1.0, 4.5): event 0's from lies between: 0.5, not 0.5 * 0.1
    assert k.Observe([1.0, 1.0, 1.0, 4.5]) == pytest.approx(0.5 * SIMIL.Observe([1.0, 1.0, 1.0, 4.5]))


def test_events_axis_and_matrix_walk():
    ev = [(0.0, 0.5, 0.3), (-1.0, 2.0, 0.6)]
    k = kernel.Events(SIMIL, ev, axis=1)
    xa, xb = [0.2, -0.2, 9.0], [0.3, 0.7, -4.0]
    x = [1.2, 0.8] + xa + xb
    assert k.Observe(x) == pytest.approx(0.3 * SIMIL.Observe(x))
    rng = np.random.default_rng(3)
    a, b = rng.uniform(-2, 3, 40), rng.uniform(-2, 3, 30)
    a[:3] = [0.0, 0.5, 2.0]
    b[:3] = [0.5, 0.0, -1.0]
    D = R.discount_matrix(ev, a, b)
    for i in range(len(a)):
        for j in range(len(b)):
            assert D[i, j] == R.discount_pair(ev, a[i], b[j])


def test_events_constructor_refusals():
    with pytest.raises(ValueError):
        kernel.Events(SIMIL, [(0.0, 1.0)])
    with pytest.raises(ValueError):
        kernel.Events(SIMIL, [(0.0, 1.0, 0.5)] * 33)
    with pytest.raises(ValueError):
        kernel.Events(SIMIL, [(0.0, math.nan, 0.5)])
    with pytest.raises(ValueError):
        kernel.Events(kernel.ARD(kernel.Normal, 2), [(0.0, 1.0, 0.5)])
    with pytest.raises(ValueError):
        kernel.Events(kernel.Events(SIMIL, [(0.0, 1.0, 0.5)]), [(0.0, 1.0, 0.5)])
    # the wrapped kernel is unchanged
    kernel.Events(SIMIL, [(0.0, 1.0, 0.5)])
    assert SIMIL.events == []


def test_combinators_keep_or_refuse_events():
    """The discount multiplies the whole similarity: Scaled and PeriodScaled keep a wrapped kernel's events (c * f * d
    in either order); ARD and Sum cannot and refuse it -- never a silently undiscounted kernel."""
    ev = [(0.0, 1.0, 0.5), (1.5, 2.0, 0.25)]
    inner = kernel.Scaled(kernel.Events(kernel.Matern52, ev))
    outer = kernel.Events(SIMIL, ev)
    assert inner.events == outer.events and inner.event_axis == outer.event_axis == 0
    assert inner.NTheta() == outer.NTheta() == 2
    for xa, xb in ((-0.5, 0.5), (0.5, 1.7), (1.2, 1.4), (3.0, -1.0)):
        x = [1.3, 0.8, xa, xb]
        assert inner.Observe(x) == outer.Observe(x)
    assert inner.Observe([1.3, 0.8, -0.5, 0.5]) == pytest.approx(0.5 * SIMIL.Observe([1.3, 0.8, -0.5, 0.5]))
    d = kernel.build_desc(1, inner, kernel.UniformNoise)
    assert d.nterms == 1 and d.terms[0].scale_idx == 0 and d.terms[0].len_idx == 1
    on_axis = kernel.Scaled(kernel.Events(kernel.Matern52, ev, axis=1))
    assert on_axis.event_axis == 1
    per = kernel.PeriodScaled(kernel.Events(kernel.Periodic, ev), 10.0)
    assert per.events == ev
    x = [0.7, 0.4, -0.5, 0.5]
    assert per.Observe(x) == pytest.approx(0.5 * kernel.PeriodScaled(kernel.Periodic, 10.0).Observe(x))
    with pytest.raises(ValueError):
        kernel.ARD(kernel.Events(kernel.Matern52, ev), 2)
    with pytest.raises(ValueError):
        kernel.Sum([kernel.Events(SIMIL, ev), kernel.Scaled(kernel.Periodic)])
    with pytest.raises(ValueError):
        kernel.Sum([kernel.Scaled(kernel.Periodic), kernel.Events(SIMIL, ev)], order=[0, 1, 2, 3, 4])
    # without events the combinators are as before
    assert kernel.Scaled(kernel.Matern52).events == [] and kernel.Sum([SIMIL, SIMIL]).events == []


def test_parse_events_selfcheck():
    assert kernel.parse_events(R.SELFCHECK) == [(1.0, 1.0, 0.5), (4.2, 6.7, 0.25)]
    assert kernel.parse_events("1.:2.5:0.3,3:6:0.5") == [(1.0, 2.5, 0.3), (3.0, 6.0, 0.5)]  # main.go:32-33
    assert kernel.parse_events("") == []
    with pytest.raises(ValueError):
        kernel.parse_events("1:2")
    with pytest.raises(ValueError):
        kernel.parse_events("1:x:0.5")


def test_events_check_refusals():
    from gogp_amd import _lib
    L = _lib.lib()
    from gogp_amd.gp import _dp
    ev = np.array([[1.0, 1.0, 0.5], [4.2, 6.7, 0.25]])
    assert L.gogp_events_check(_dp(ev), 2, 0, 1) == _lib.GOGP_OK
    assert L.gogp_events_check(None, 0, 0, 1) == _lib.GOGP_OK  # no events
    many = np.zeros((33, 3))
    assert L.gogp_events_check(_dp(many), 33, 0, 1) == _lib.GOGP_EARG
    assert L.gogp_events_check(_dp(many), 32, 0, 1) == _lib.GOGP_OK
    assert L.gogp_events_check(_dp(ev), 2, 1, 1) == _lib.GOGP_EARG  # axis >= ndim
    assert L.gogp_events_check(_dp(ev), 2, -1, 3) == _lib.GOGP_EARG
    assert L.gogp_events_check(_dp(ev), 2, 2, 3) == _lib.GOGP_OK
    assert L.gogp_events_check(_dp(ev), -1, 0, 1) == _lib.GOGP_EARG
    for bad in (math.nan, math.inf, -math.inf):
        for f in range(3):
            e = ev.copy()
            e[1, f] = bad
            assert L.gogp_events_check(_dp(e), 2, 0, 1) == _lib.GOGP_EARG
    assert L.gogp_events_check(None, 2, 0, 1) == _lib.GOGP_EARG


def test_restatement_gradient_matches_its_own_fd(golden_dir):
    import os
    data = np.loadtxt(os.path.join(golden_dir, "events.csv"), delimiter=",")
    X, y = data[:, :1], (data[:, 1] - data[:, 1].mean()) / data[:, 1].std(ddof=1)
    g = R.RefGP(1, kernel.parse_events(R.SELFCHECK))
    g.X, g.Y = X, y
    x = np.log([1.3, 0.8, 0.6])
    g.Observe(x)
    grad = g.Gradient()
    h = 1e-5
    for p in range(3):
        e = np.zeros(3)
        e[p] = h
        fd = (g.Observe(x + e) - g.Observe(x - e)) / (2 * h)
        assert abs(fd - grad[p]) <= 1e-6 * max(1.0, abs(grad[p])), (p, fd, grad[p])
