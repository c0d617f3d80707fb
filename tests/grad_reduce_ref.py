"""Host references of the kernels that turn K^-1 into the gradient (gogp_amd/csrc/grad.hip, grad_mfma.hip): the slot sums
of the fused reduction and the input gradient, written from the formulas of the similarity kernels (kern_eval.h's header:
kernel/kernel.go:23-26, 44-47, 70-73, 89-92), not from the device code.

With W_ij = alpha_i alpha_j - Kinv_ij read from the LOWER triangle (j <= i < n, off-diagonal pairs counted twice: weight
m_ij = 2, diagonal 1) and d_ij the pair's event discount, term t = c f(.) contributes per pair, to the slots of common.h,

    radial kinds, s = sum_d ((x_id - x_jd) / l_d)^2:
        slot 3t      m W d  c f(s)                                  theta dk/dtheta for the output scale
        slot 3t + 1  m W d  c (-2 f'(s)) s                          one length scale: ds/dlog l = -2 s
        slot 16 + d  m W d  c (-2 f'(s)) ((x_id - x_jd) / l_d)^2    ARD: ds/dlog l_d = -2 u_d^2
    periodic, phi_d = w |x_id - x_jd|, s = sum_d (sin phi_d / l_d)^2, f = exp(-2 s):
        slot 3t      m W d  c f
        slot 3t + 1  m W d  c f 4 s              (ARD: slot 16 + d, 4 (sin phi_d / l_d)^2)
        slot 3t + 2  m W d  c f 4 sum_d sin phi_d cos phi_d phi_d / l_d^2        dphi/dlog p = -phi
    slot 12          sum_i W_ii                  (the noise on the diagonal; no discount)

and the input gradient gx[i][d] = sum_{j != i} W_ij d_ij dk(x_i, x_j)/dx_id over the FULL symmetric W, with
dk/dx_id = c f'(s) 2 (x_id - x_jd) / l_d^2 (radial) and -4 c f w sin phi_d cos phi_d sign(x_id - x_jd) / l_d^2 (periodic).

Modes:
- "ld": numpy.longdouble values, and beside each a RUNNING ERROR BOUND e_q for an fp64 evaluation of the same sums in any
  order.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 3.1).
  A slot is a sum of m terms T (one per pair): e_q = gamma_m sum |T| + sum |T| rho, rho the pair's first-order relative
  error, which has three parts:
    * 2 u for forming W (the product and the difference; one rounding where they are fused),
    * the error of s times the slot function's condition number at s.  The kernels that difference per pair err by
      gamma_{D+2} s.  The matrix-core form of grad_mfma.hip expands r^2 = |a|^2 + |b|^2 - 2 a.b with a = (x_i - x_ref) / l,
      b = (x_j - x_ref) / l centred on the first column point of the pair's 64-column tile (row min(64 floor(j / 64),
      n - 1)): it errs by gamma_{DP+4} (|a|^2 + |b|^2 + 2 |a| |b|), DP = D rounded up to 16.  Its ARD sums are expanded the
      same way (sum g a_d^2 + sum g b_d^2 - 2 sum g a_d b_d), so there the slot's terms -- the |T| of gamma_m sum |T| --
      are those three per pair: |g| (|a_d| + |b_d|)^2.  (The bound is written in absolute form, |h'(s)| ds, so that a
      pair with h(s) = 0 needs no division; on the diagonal s = 0 and u_d = 0 exactly.)
    * eps_fn per transcendental call (exp; sqrt and exp for the Matern kinds; sin, cos and exp for the periodic one).
      The device math library's accuracy table is not among this repository's documents: eps_fn = 4 u is ASSUMED
      (the OpenCL full-profile limits for double exp, sin and cos are 3, 4 and 4 ulp).
  The bound's own sums run in float64 on non-negative terms and are inflated by 1 + 2^-30.  It comes from this model and
  the inputs only.
- "f64": the same formulas in plain float64 -- the run the bound is about (tests/test_grad_reduce_ref_cpu.py).
- exact (exact_slots): every row of X identical, so r^2 = 0 and f = 1 for every pair and exp, sqrt, sin of 0 are exact;
  alpha and Kinv small integers, c a power of two.  Slot 3t = c sum m_ij W_ij and slot 12 = sum W_ii are integers below
  2^53 in any summation order (asserted from the absolute sums); every other slot is exactly 0.  A kernel must return
  these bit for bit: this pins WHICH elements are read with WHICH weight.
"""
import numpy as np

from cases import NAN32, NAN64  # noqa: F401  (the tests take the sentinels from here)

U = 2.0 ** -53
EPS_FN = 4 * U
_INFLATE = 1.0 + 2.0 ** -30
NACC, ACC_TRACE, ACC_ARD0 = 80, 12, 16
MAX_TERMS, MAX_NDIM, MAX_EVENTS = 4, 64, 32
K_NORMAL, K_MATERN32, K_MATERN52, K_MATERN52_TEXTBOOK, K_PERIODIC = range(5)
LD = np.longdouble
SQRT3, SQRT5 = 1.7320508075688772, 2.2360679774997900  # kernel/kernel.go:51-52, the literals


def gamma(k):
    return k * U / (1.0 - k * U)


class KP:
    """The kernel's parameters as the device sees them.  terms: dicts with kind, ard (False), c (1.0), w (0.0: pi / period)
    and inv_len (a number or ndim numbers: 1 / l_d); events: (from, to, discount) triples on coordinate ev_axis."""

    def __init__(self, ndim, terms, events=(), ev_axis=0, noise_var=0.0, dnoise=0.0):
        self.ndim, self.events, self.ev_axis, self.noise_var, self.dnoise = ndim, list(events), ev_axis, noise_var, dnoise
        self.terms = [dict(kind=int(T["kind"]), ard=bool(T.get("ard", False)), c=float(T.get("c", 1.0)),
                           w=float(T.get("w", 0.0)),
                           inv_len=np.broadcast_to(np.asarray(T.get("inv_len", 1.0), float), (ndim,)).copy()) for T in terms]

    @property
    def ard_dims(self):
        return self.ndim if any(T["ard"] for T in self.terms) else 0

    @property
    def radial1(self):
        return len(self.terms) == 1 and self.terms[0]["kind"] != K_PERIODIC

    def hook(self, gp):
        return gp.kparams(self.ndim, self.terms, self.noise_var, self.dnoise, self.events, self.ev_axis)


def kp_from_desc(desc, ts, tn=()):
    """KP of a descriptor (gogp_amd.kernel.build_desc) at the natural parameters ts, tn."""
    terms = []
    for t in range(desc.nterms):
        T = desc.terms[t]
        il = [1.0 / ts[T.len_idx + (j if T.ard else 0)] for j in range(desc.ndim)]
        terms.append(dict(kind=T.kind, ard=bool(T.ard), c=ts[T.scale_idx] if T.scale_idx >= 0 else 1.0, inv_len=il,
                          w=np.pi / (T.period_mult * ts[T.period_idx]) if T.kind == K_PERIODIC else 0.0))
    if desc.noise_kind in (0, 2):
        nv, dn = desc.noise_std ** 2, 0.0
    else:
        nv = desc.noise_scale * tn[0] ** 2
        dn = 2.0 * nv
    return KP(desc.ndim, terms, noise_var=nv, dnoise=dn)


def assemble(desc, slots, dnoise):
    """d LML / d log theta from the slot sums: 0.5 * slot for every similarity parameter (scale 3t, length 3t + 1 or the
    ARD slots 16 + d, period 3t + 2), 0.5 * trace * dnoise for the noise parameter (dnoise = d noise_var / d log std)."""
    nn = 0 if desc.noise_kind == 0 else 1
    out = np.zeros(desc.ntheta_simil + nn, slots.dtype)
    for t in range(desc.nterms):
        T = desc.terms[t]
        if T.scale_idx >= 0:
            out[T.scale_idx] += 0.5 * slots[3 * t]
        if T.ard:
            for j in range(desc.ndim):
                out[T.len_idx + j] += 0.5 * slots[ACC_ARD0 + j]
        else:
            out[T.len_idx] += 0.5 * slots[3 * t + 1]
        if T.kind == K_PERIODIC:
            out[T.period_idx] += 0.5 * slots[3 * t + 2]
    if nn:
        out[desc.ntheta_simil] = 0.5 * slots[ACC_TRACE] * dnoise
    return out


def discount(events, xa, xb):
    """Discount of every pair of xa (m,) x xb (n,): an event separates a pair when exactly one of the two points lies
    below its `from`, or exactly one below its `to`; the first such event in list order sets the factor."""
    d = np.ones((len(xa), len(xb)))
    if not len(events):
        return d
    sep = np.stack([((xa[:, None] < frm) != (xb[None, :] < frm)) | ((xa[:, None] < to) != (xb[None, :] < to))
                    for frm, to, _ in events])
    first = sep.argmax(0)
    disc = np.array([e[2] for e in events], float)
    return np.where(sep.any(0), disc[first], d)


def _radial(kind, s, dt):
    """f(s), f'(s) and f''(s) s of a radial kind (s = r^2)."""
    if kind == K_NORMAL:
        f = np.exp(-s / 2)
        return f, -f / 2, f * s / 4
    r = np.sqrt(s)
    a = dt(SQRT3 if kind == K_MATERN32 else SQRT5)
    e = np.exp(-a * r)
    if kind == K_MATERN32:
        return (1 + a * r) * e, -(a * a / 2) * e, (a * a * a / 4) * e * r
    q = dt(1) if kind == K_MATERN52 else dt(5) / dt(3)  # kernel/kernel.go:89-92: Go's 5 / 3 is 1
    f1 = (q - a * a / 2 - q * a * r / 2) * e
    return (1 + a * r + q * s) * e, f1, e * r * (-q * a / 4 - (q - a * a / 2) * a / 2 + q * a * a * r / 4)


def _f64(a):
    return np.abs(a).astype(np.float64)


def ref_rows(n):
    """Row whose coordinates centre column j's tile in grad_mfma.hip."""
    return np.minimum(64 * (np.arange(n) // 64), n - 1)


class _Acc:
    def __init__(self, Ws, dt, shape, m, n):
        self.n = n
        self.W = Ws
        self.A = [_f64(w) for w in Ws]
        self.val = np.zeros((len(Ws),) + shape, dt)
        self.bnd = np.zeros((len(Ws),) + shape)
        self.m = m

    def add(self, idx, M, EM, Mabs=None, axis=None):
        g = gamma((3 if Mabs is not None else 1) * self.m + 8) + 2 * U
        Ma = _f64(M) if Mabs is None else Mabs
        for k, (w, a) in enumerate(zip(self.W, self.A)):
            self.val[k][idx] += (w * M).sum(axis)
            self.bnd[k][idx] += (g * (a * Ma).sum(axis) + (a * EM).sum(axis)) * _INFLATE


def _pair_terms(kp, X, n, acc, form, dt, xgrad, rows=None, cols=None):
    """Every term's per-pair factors, for the pairs rows x cols (global indices below n; default all), into acc (slot
    sums, or with xgrad the input gradient per (i, d))."""
    D = kp.ndim
    rows = np.arange(n) if rows is None else rows
    cols = np.arange(n) if cols is None else cols
    Xa, Xb = X[rows].astype(dt), X[cols].astype(dt)
    diff = lambda d: Xa[:, None, d] - Xb[None, :, d]  # noqa: E731
    n, shape = None, (len(rows), len(cols))
    for t, T in enumerate(kp.terms):
        c, ac, il, kind = dt(T["c"]), abs(T["c"]), T["inv_len"].astype(dt), T["kind"]
        ilf = T["inv_len"]
        if kind != K_PERIODIC:
            s = np.zeros(shape, dt)
            for d in range(D):
                s += (diff(d) * il[d]) ** 2
            sf = s.astype(np.float64)
            if form == "mfma":
                ref = ref_rows(acc.n)[cols]
                A = [(X[rows, None, d] - X[ref, d][None, :]) * ilf[d] for d in range(D)]   # a_d of pair (i, j)
                B = [(X[cols, d] - X[ref, d]) * ilf[d] for d in range(D)]                  # b_d of column j
                na = np.sqrt(sum(a * a for a in A))
                nb = np.sqrt(sum(b * b for b in B))[None, :]
                ds = gamma((D + 15) // 16 * 16 + 4) * (na + nb) ** 2
            else:
                ds = gamma(D + 2) * sf
            f, f1, f2s = _radial(kind, s, dt)
            ff, f1f, f2sf = _f64(f), _f64(f1), _f64(f2s)
            f2f = np.divide(f2sf, sf, out=np.zeros_like(sf), where=sf > 0)
            efn = (1 if kind == K_NORMAL else 2) * EPS_FN
            if xgrad:
                for d in range(D):
                    M = 2 * c * f1 * diff(d) * il[d] ** 2
                    acc.add((slice(None), d), M, _f64(M) * (efn + 4 * U) + 2 * ac * f2f * ds * _f64(diff(d)) * ilf[d] ** 2,
                            axis=1)
                continue
            acc.add(3 * t, c * f, ac * (ff * efn + f1f * ds))
            if not T["ard"]:
                M = -2 * c * f1 * s
                acc.add(3 * t + 1, M, _f64(M) * (efn + 2 * U) + 2 * ac * _f64(f2s + f1) * ds)
                continue
            for d in range(D):
                u2 = (diff(d) * il[d]) ** 2
                M = -2 * c * f1 * u2
                EM = _f64(M) * (efn + 4 * U) + 2 * ac * f2f * ds * _f64(u2)
                acc.add(ACC_ARD0 + d, M, EM, 2 * ac * f1f * (np.abs(A[d]) + np.abs(B[d])[None, :]) ** 2 if form == "mfma"
                        else None)
            continue
        # periodic
        w = dt(T["w"])
        s, gp, dsn, dgp, gpa = np.zeros(shape, dt), np.zeros(shape, dt), np.zeros(shape), np.zeros(shape), np.zeros(shape)
        per_d = []
        for d in range(D):
            phi = w * np.abs(diff(d))
            sn, cs = np.sin(phi), np.cos(phi)
            dd2 = (sn * il[d]) ** 2
            s += dd2
            gterm = sn * cs * phi * il[d] ** 2
            gp += gterm
            phf = _f64(phi)
            ddd = 2 * _f64(sn) * ilf[d] ** 2 * (_f64(cs) * phf * 2 * U + _f64(sn) * EPS_FN) + 3 * U * _f64(dd2)
            dsn += ddd
            gpa += _f64(gterm)
            dgp += ilf[d] ** 2 * (_f64(sn * cs) * phf * (2 * EPS_FN + 4 * U)
                                  + _f64(np.cos(2 * phi) * phi + sn * cs) * phf * 2 * U)
            per_d.append((dd2, ddd, sn, cs))
        ds = dsn + gamma(D) * _f64(s)
        dgp += gamma(D) * gpa
        f = np.exp(-2 * s)
        ff = _f64(f)
        if xgrad:
            for d in range(D):
                _, _, sn, cs = per_d[d]
                dx = diff(d)
                M = -4 * c * f * w * sn * cs * np.sign(dx) * il[d] ** 2
                phf = _f64(w * np.abs(dx))
                EM = (_f64(M) * (3 * EPS_FN + 6 * U + 2 * ds)
                      + 4 * ac * ff * abs(T["w"]) * ilf[d] ** 2 * _f64(np.cos(2 * w * np.abs(dx))) * phf * 2 * U)
                acc.add((slice(None), d), M, EM, axis=1)
            continue
        acc.add(3 * t, c * f, ac * ff * (EPS_FN + 2 * ds))
        M = 4 * c * f * gp
        acc.add(3 * t + 2, M, _f64(M) * (EPS_FN + 2 * U + 2 * ds) + 4 * ac * ff * dgp)
        if not T["ard"]:
            M = 4 * c * f * s
            acc.add(3 * t + 1, M, _f64(M) * (EPS_FN + 2 * U) + 4 * ac * ff * _f64(1 - 2 * s) * ds)
        else:
            for d in range(D):
                dd2, ddd, _, _ = per_d[d]
                M = 4 * c * f * dd2
                acc.add(ACC_ARD0 + d, M, _f64(M) * (EPS_FN + 2 * U + 2 * ds) + 4 * ac * ff * ddd)


def slot_sums(kp, X, n, alpha, Kinvs, rows=None, cols=None, form="diff", mode="ld"):
    """The NACC slot sums over the pairs (i, j), j <= i, of rows x cols (global indices below n; default the whole lower
    triangle) for every Kinv of the list Kinvs (arrays of shape (len(rows), len(cols)) holding Kinv[rows][:, cols];
    float32 ones are widened; elements with j > i are not used).  X: (>= n, D), alpha: (>= n,).  Returns (vals, bounds),
    each (len(Kinvs), NACC): long doubles and the float64 e_q in mode "ld", plain float64 values (and the same bounds)
    in mode "f64"."""
    assert mode in ("ld", "f64") and form in ("diff", "mfma")
    dt = LD if mode == "ld" else np.float64
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    mask = cols[None, :] <= rows[:, None]
    dg = cols[None, :] == rows[:, None]
    mult = np.where(dg, 1, 2) * mask
    a = alpha.astype(dt)
    Ws = [np.where(mask, np.outer(a[rows], a[cols]) - np.where(mask, K, 0).astype(dt), 0) for K in Kinvs]
    disc = discount(kp.events, X[rows, kp.ev_axis], X[cols, kp.ev_axis]).astype(dt)
    acc = _Acc([W * mult * disc for W in Ws], dt, (NACC,), int(mask.sum()), n)
    _pair_terms(kp, X, n, acc, form, dt, False, rows, cols)
    for k, W in enumerate(Ws):
        acc.val[k][ACC_TRACE] = W[dg].sum()
        acc.bnd[k][ACC_TRACE] = (gamma(int(dg.sum()) + 8) + 2 * U) * _f64(W[dg]).sum() * _INFLATE
    return acc.val, acc.bnd


def xgrad_sums(kp, X, n, alpha, Ksym, mode="ld"):
    """gx (n, D) over the full symmetric W = alpha alpha^T - Ksym (its diagonal is not used) and its bound."""
    dt = LD if mode == "ld" else np.float64
    a = alpha[:n].astype(dt)
    W = np.outer(a, a) - Ksym[:n, :n].astype(dt)
    np.fill_diagonal(W, 0)
    W = W * discount(kp.events, X[:n, kp.ev_axis], X[:n, kp.ev_axis]).astype(dt)
    acc = _Acc([W], dt, (n, kp.ndim), (n - 1) * len(kp.terms), n)
    _pair_terms(kp, X, n, acc, "diff", dt, True)
    return acc.val[0], acc.bnd[0]


def exact_slots(kp, alpha, Kinv, n, mask=None, as_object=False):
    # (mask: boolean (n, n); tile_mask gives a rank's)
    """Exact mode: the slot sums for identical rows of X (f = 1, discount 1), integer alpha and Kinv and c a power of two,
    as float64 -- after asserting that the absolute sums stay below 2^53, so that any summation order gives these bits.
    as_object: the integers themselves (Python ints; slot 3t WITHOUT the factor c), to check the int64 run against."""
    low = np.tril(np.ones((n, n), bool))
    mask = low if mask is None else (mask & low)
    a, K = alpha[:n], Kinv[:n, :n]
    assert np.array_equal(a, np.rint(a)) and np.array_equal(K[mask], np.rint(K[mask])), "exact mode needs integers"
    it = object if as_object else np.int64
    ai = a.astype(np.int64).astype(it)
    W = np.where(mask, np.outer(ai, ai) - np.where(mask, K, 0).astype(np.int64).astype(it), 0)
    mult = np.where(np.eye(n, dtype=bool), 1, 2)
    total, trace = (W * mult).sum(), np.diag(W)[np.diag(mask)].sum() if np.diag(mask).any() else 0
    cmax = max(abs(T["c"]) for T in kp.terms)
    head = float(np.abs(W.astype(np.float64) * mult).sum()) * max(cmax, 1.0)
    assert head < 2.0 ** 53, "a partial sum may reach 2^%.1f" % np.log2(head)
    if as_object:
        return int(total), int(trace)
    out = np.zeros(NACC)
    for t, T in enumerate(kp.terms):
        m, e = np.frexp(T["c"])
        assert m == 0.5, "c must be a power of two"
        out[3 * t] = T["c"] * float(total)
    out[ACC_TRACE] = float(trace)
    return out


def tile_mask(n, grid=None, nb=512, npad=None):
    """Pairs (i, j) of the lower triangle that the launch reads: all of it, or with grid = (pr, Pr, pc, Pc) those whose
    row block (of nb) belongs to grid row pr and whose column block to grid column pc, in 64 x 64 tiles that are not
    wholly above the diagonal (tile column start <= tile row start)."""
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    m = (j <= i)
    if grid is not None:
        pr, Pr, pc, Pc = grid
        m = m & ((i // nb) % Pr == pr) & ((j // nb) % Pc == pc)
    return m
