"""Host references of the kernels that consume the factor (gogp_amd/csrc/trsm_small.hip and, of solve.hip, the
substitution steps), the solution layouts of the one-pass kernel, and the operands the tests feed them.

The blocked recurrences are written as the kernels define them -- with the GIVEN 256-block inverses, not a solve with the
true diagonal block (nb = npad / 256 blocks):

    forward:   w_B = b_B - sum_{j < B} L[B, j] v_j ,        v_B = Dinv_B w_B          (B = 0 .. nb - 1)
    backward:  w_B = b_B - sum_{j > B} L[j, B]^T v_j ,      v_B = Dinv_B^T w_B        (B = nb - 1 .. 0)

Two modes:
- "int": integer operands, integer arithmetic -- exact values.  The recurrence runs on int64 after asserting, from
  |Dinv_B| (|b_B| + sum_j |L_Bj| |v_j|), that every partial sum taken in ANY order, over absolute values even, stays
  below 2^53: then int64 cannot overflow, and an fp64 kernel that sums in whatever order must return these integers bit
  for bit.  ("object": the same on Python ints, to check the int64 run against.)
- "ld": numpy.longdouble values and a RUNNING ERROR BOUND for an fp64 evaluation of the same recurrence in any order.
  With u = 2^-53 and gamma_k = k u / (1 - k u), a dot product of k terms summed in any order (each product rounded, or
  fused: FMA and MFMA chains only tighten it) errs by at most gamma_k sum |terms| (Higham, Accuracy and Stability of
  Numerical Algorithms, 2nd ed., section 3.1).  w_B is one such sum of 256 B + 1 terms whose operands v_j carry the
  errors e_j, v_B one of 256 terms whose operand w_B carries ew_B:
      ew_B = gamma_{256 B + 2} (|b_B| + sum_j |L_Bj| |v_j|) + sum_j |L_Bj| e_j
      e_B  = gamma_{258} |Dinv_B| |w_B| + |Dinv_B| ew_B
  The bound's own sums run in float64 BLAS on non-negative terms (relative error below 2^-40) and are inflated by
  1 + 2^-30; the long-double values are off by some 2^-64 relative, far inside it.
"""
import functools

import numpy as np

from cases import NAN32, NAN64  # noqa: F401  (the tests take the sentinels from here)

P = 256
U = 2.0 ** -53
TS_SOL_PAIRED, TS_SOL_COMPACT, TS_SOL_GRANULE = 0, 1, 2
_INFLATE = 1.0 + 2.0 ** -30


def gamma(k):
    return k * U / (1.0 - k * U)


def _blocks(npad):
    assert npad % P == 0 and npad > 0
    return npad // P


def _blk(L, B, j, backward):
    """The block that multiplies v_j in the rows of block B."""
    if backward:
        return L[j * P:(j + 1) * P, B * P:(B + 1) * P].T
    return L[B * P:(B + 1) * P, j * P:(j + 1) * P]


def substitute(L, Dinv, b, mode="ld", backward=False):
    """The blocked recurrence.  L: (npad, npad), only the blocks strictly below the diagonal are read; Dinv: (nb, 256,
    256); b: (npad, m) right-hand sides as columns.  Returns (V, W) -- exact integers (int64 / object arrays) -- in the
    integer modes (and plain float64 in mode "f64", the run the bound is about) and (V, W, E, EW) -- long doubles, and
    the float64 bounds on |V_fp64 - V| and |W_fp64 - W| -- in mode "ld"."""
    npad, m = b.shape
    nb = _blocks(npad)
    assert L.shape == (npad, npad) and Dinv.shape == (nb, P, P)
    order = range(nb - 1, -1, -1) if backward else range(nb)
    if mode in ("int", "object"):
        for a in (L, Dinv, b):
            assert np.array_equal(a, np.rint(a)), "integer modes need integer operands"
        it = np.int64 if mode == "int" else object
        cast = (lambda a: a.astype(np.int64)) if mode == "int" else (lambda a: a.astype(np.int64).astype(object))
    else:
        assert mode in ("ld", "f64")
        it = np.longdouble if mode == "ld" else np.float64
        cast = lambda a: a.astype(it)  # noqa: E731
    V, W = np.zeros((npad, m), it), np.zeros((npad, m), it)
    Vabs = np.zeros((npad, m))  # |v| in float64 (the bound's sums and the headroom check)
    E, EW = np.zeros((npad, m)), np.zeros((npad, m))
    done = []
    for B in order:
        rows = slice(B * P, (B + 1) * P)
        D = Dinv[B].T if backward else Dinv[B]
        w = cast(b[rows])
        mag = np.abs(b[rows]).astype(np.float64)
        ein = np.zeros((P, m))
        for j in done:
            cols = slice(j * P, (j + 1) * P)
            Lb = _blk(L, B, j, backward)
            w = w - cast(Lb) @ V[cols]
            La = np.abs(Lb).astype(np.float64)
            mag += La @ Vabs[cols]
            if mode == "ld":
                ein += La @ E[cols]
        v = cast(D) @ w
        Da = np.abs(D).astype(np.float64)
        if mode in ("int", "object"):
            head = (Da @ mag).max()
            assert head < 2.0 ** 53, "a partial sum may reach 2^%.1f: no 2^53 headroom" % np.log2(head)
        elif mode == "ld":
            ew = EW[rows] = (gamma(P * len(done) + 2) * mag + ein) * _INFLATE
            E[rows] = (gamma(P + 2) * (Da @ np.abs(w).astype(np.float64)) + Da @ ew) * _INFLATE
        V[rows], W[rows] = v, w
        Vabs[rows] = np.abs(v).astype(np.float64)
        done.append(B)
    return (V, W, E, EW) if mode == "ld" else (V, W)


def fwd_step(L, Dinv, bk, w, mode="ld"):
    """One forward step of solve.hip on one right-hand side: z_b = Dinv_b w_b; w_i -= L[i, b] z_b for the rows below
    block b.  Returns (z_b, w_new) -- and, in mode "ld", the bounds (ez, ew) of an fp64 evaluation: z_b a 256-term dot
    product, every updated w_i one of 257 terms whose operand z_b carries ez."""
    npad = w.shape[0]
    rows, below = slice(bk * P, (bk + 1) * P), slice((bk + 1) * P, npad)
    it = np.int64 if mode == "int" else np.longdouble
    Lb = L[below, rows]
    z = Dinv[bk].astype(it) @ w[rows].astype(it)
    wn = w.astype(it)
    wn[below] -= Lb.astype(it) @ z
    if mode == "int":
        head = max((np.abs(Dinv[bk]) @ np.abs(w[rows])).max(),
                   (np.abs(w[below]) + np.abs(Lb) @ np.abs(z).astype(np.float64)).max(initial=0.0))
        assert head < 2.0 ** 53
        return z, wn
    Da, La = np.abs(Dinv[bk]).astype(np.float64), np.abs(Lb).astype(np.float64)
    za = np.abs(z).astype(np.float64)
    ez = gamma(P + 2) * (Da @ np.abs(w[rows])) * _INFLATE
    ew = np.zeros(npad)
    ew[below] = (gamma(P + 2) * (np.abs(w[below]) + La @ za) + La @ ez) * _INFLATE
    return z, wn, ez, ew


def bwd_step(L, Dinv, bk, w, mode="ld"):
    """One backward step: alpha_b = Dinv_b^T w_b; w_i -= L[b, i]^T alpha_b for the rows above block b."""
    npad = w.shape[0]
    rows, above = slice(bk * P, (bk + 1) * P), slice(0, bk * P)
    it = np.int64 if mode == "int" else np.longdouble
    Lb = L[rows, above].T
    a = Dinv[bk].T.astype(it) @ w[rows].astype(it)
    wn = w.astype(it)
    wn[above] -= Lb.astype(it) @ a
    if mode == "int":
        head = max((np.abs(Dinv[bk].T) @ np.abs(w[rows])).max(),
                   (np.abs(w[above]) + np.abs(Lb) @ np.abs(a).astype(np.float64)).max(initial=0.0))
        assert head < 2.0 ** 53
        return a, wn
    Da, La = np.abs(Dinv[bk].T).astype(np.float64), np.abs(Lb).astype(np.float64)
    aa = np.abs(a).astype(np.float64)
    ea = gamma(P + 2) * (Da @ np.abs(w[rows])) * _INFLATE
    ew = np.zeros(npad)
    ew[above] = (gamma(P + 2) * (np.abs(w[above]) + La @ aa) + La @ ea) * _INFLATE
    return a, wn, ea, ew


def sumsq_exact(V):
    """Column sums of squares of an integer solution, exactly (Python ints), as floats rounded once."""
    Vo = V.astype(object)
    return np.array([float(sum(int(x) * int(x) for x in Vo[:, j])) for j in range(V.shape[1])])


# ---- operands ----------------------------------------------------------------------------------------------------------
def exact_operands(npad, m, seed):
    """Dense integer operands: L and Dinv entries in {-1, 0, 1} (Dinv lower triangular, its upper triangle exactly
    zero), right-hand sides integers in [-8, 8].  All representable in float.  Only the blocks of L strictly below the
    diagonal are filled; the rest is zero here (the tests put sentinels there)."""
    rng = np.random.default_rng(seed)
    nb = _blocks(npad)
    L = np.zeros((npad, npad))
    for B in range(1, nb):
        L[B * P:(B + 1) * P, :B * P] = rng.integers(-1, 2, (P, B * P))
    Dinv = np.tril(rng.integers(-1, 2, (nb, P, P))).astype(np.float64)
    b = rng.integers(-8, 9, (npad, m)).astype(np.float64)
    return L, Dinv, b


def mantissa_operands(npad, m, seed, as_float=False, lscale=None):
    """Full-mantissa operands: L blocks uniform(-1, 1) lscale / sqrt(npad), Dinv blocks the fp64 inverse of I plus a small
    strictly lower part (upper triangle exactly zero), normal right-hand sides.  as_float: everything rounded to float
    (and returned as float64 values that floats hold exactly).  lscale: 1 up to npad = 1280, 1 / 8 beyond -- the running
    bound sums ABSOLUTE values, which grow by 1 + 128 lscale / sqrt(npad) per block where the signed sums stay O(1); at
    npad = 4352 the unscaled operands push it to 1e-5 of max |V|, past the 1e-10 the tests require of it."""
    if lscale is None:
        lscale = 1.0 if npad <= 1280 else 0.125
    rng = np.random.default_rng(seed)
    nb = _blocks(npad)
    L = np.zeros((npad, npad))
    for B in range(1, nb):
        L[B * P:(B + 1) * P, :B * P] = rng.uniform(-1, 1, (P, B * P)) * (lscale / np.sqrt(npad))
    Dinv = np.empty((nb, P, P))
    for B in range(nb):
        T = np.eye(P) + np.tril(rng.uniform(-1, 1, (P, P)), -1) / P
        Dinv[B] = np.tril(np.linalg.inv(T))
    b = rng.standard_normal((npad, m))
    if as_float:
        L, Dinv, b = (a.astype(np.float32).astype(np.float64) for a in (L, Dinv, b))
    return L, Dinv, b


# ---- the solution layouts of the one-pass kernel (common.h: TS_SOL_*) -----------------------------------------------
def encode_paired(V, width):
    """Element (row k, rhs j) at ((k >> 1) * width + j) * 2 + (k & 1) doubles."""
    npad, m = V.shape
    assert npad % 2 == 0 and m <= width
    full = np.zeros((npad, width))
    full[:, :m] = V
    return np.ascontiguousarray(full.reshape(npad // 2, 2, width).transpose(0, 2, 1)).reshape(-1).view(np.uint8)


def decode_paired(raw, npad, width):
    a = np.frombuffer(raw, np.float64, npad * width).reshape(npad // 2, width, 2)
    return a.transpose(0, 2, 1).reshape(npad, width).copy()


def encode_compact(V, width):
    """Element (row k, rhs j) at k * width + j doubles."""
    npad, m = V.shape
    full = np.zeros((npad, width))
    full[:, :m] = V
    return full.reshape(-1).view(np.uint8)


def decode_compact(raw, npad, width):
    return np.frombuffer(raw, np.float64, npad * width).reshape(npad, width).copy()


def encode_granule(v, tag=1):
    """One right-hand side, 16 bytes per row: {tag, low word, tag, high word}."""
    bits = np.ascontiguousarray(v, dtype=np.float64).reshape(-1).view(np.uint64)
    g = np.empty((bits.size, 4), np.uint32)
    g[:, 0] = g[:, 2] = tag
    g[:, 1] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    g[:, 3] = (bits >> np.uint64(32)).astype(np.uint32)
    return g.reshape(-1).view(np.uint8)


def decode_granule(raw, npad):
    """(V as npad x 1, tags as npad x 2)."""
    g = np.frombuffer(raw, np.uint32, npad * 4).reshape(npad, 4)
    bits = g[:, 1].astype(np.uint64) | (g[:, 3].astype(np.uint64) << np.uint64(32))
    return bits.view(np.float64).reshape(npad, 1).copy(), g[:, [0, 2]].copy()


def decode_solution(ws, kind, width, sol_off, npad):
    """V (npad x width doubles) from the raw bytes of a launch's workspace, by the layout trsm_small_solution reported.
    A granule whose tags are not the launch's fails here."""
    raw = np.ascontiguousarray(ws, dtype=np.uint8)[sol_off:]
    if kind == TS_SOL_PAIRED:
        return decode_paired(raw, npad, width)
    if kind == TS_SOL_COMPACT:
        return decode_compact(raw, npad, width)
    assert kind == TS_SOL_GRANULE and width == 1, (kind, width)
    V, tags = decode_granule(raw, npad)
    assert (tags == 1).all(), "granules without the launch's tag: %d" % int((tags != 1).sum())
    return V


def expected_solution(prec, j0, cnt):
    """(instance name, kind, width) of the launch for these right-hand sides, as common.h documents them."""
    if prec == 64 and j0 == 0 and cnt == 1:
        return "granule", TS_SOL_GRANULE, 1
    for mc in (1, 2, 4, 8):
        if cnt <= mc:
            return "NT1-MC%d" % mc, TS_SOL_COMPACT, mc
    return ("NT1-MC16", TS_SOL_PAIRED, 16) if cnt <= 16 else ("NT2-MC32", TS_SOL_PAIRED, 32)


# ---- the problems the tests share: computed once, never written to ------------------------------------------------------
NPADS = (256, 512, 768, 1280)  # B = 0, B = 1, the first reuse of the operand ring at B = 2, several steps
NPAD_BIG = 4352  # 272 workgroups: more than one per compute unit for the granule kernel's 132 KB of LDS
M_MASTER, M_BIG = 64, 17
#: every random problem of tests/test_substitution_kernels.py: (npad, right-hand sides, seed, rounded to float)
MANTISSA_CASES = ([(n, M_MASTER, 7000 + n, f) for n in NPADS for f in (False, True)]
                  + [(NPAD_BIG, M_BIG, 7000 + NPAD_BIG, False)]
                  + [(768, 1, 7900 + c, False) for c in range(3)])  # the candidates of the batched forward steps


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def exact_problem(npad, m=M_MASTER, seed=None, backward=False):
    """(L, Dinv, b, V, W) of the integer problem of this size, solved exactly."""
    L, Dinv, b = exact_operands(npad, m, 5000 + npad if seed is None else seed)
    return _frozen(L, Dinv, b, *substitute(L, Dinv, b, "int", backward=backward))


@functools.lru_cache(maxsize=None)
def mantissa_problem(npad, as_float=False, m=None, seed=None, backward=False):
    """(L, Dinv, b, V, W, E, EW) of the random problem of this size (one of MANTISSA_CASES)."""
    m = (M_MASTER if npad != NPAD_BIG else M_BIG) if m is None else m
    seed = 7000 + npad if seed is None else seed
    assert (npad, m, seed, as_float) in MANTISSA_CASES or backward
    L, Dinv, b = mantissa_operands(npad, m, seed, as_float=as_float)
    return _frozen(L, Dinv, b, *substitute(L, Dinv, b, "ld", backward=backward))
