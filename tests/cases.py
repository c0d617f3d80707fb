"""Kernel families exercised by the parity tests and by the committed oracle vectors
(tests/golden/make_oracle_vectors.py): (name, NDim, Simil, Noise, theta_simil, theta_noise).

The primitives are the reference's (kernel/kernel.go:23-26,44-47,70-73,89-92,
kernel/noise.go:27-30,47-49); the compositions mirror its tutorials
(tutorial/barebones/kernel/kernel.go:14-31, tutorial/hyperpriors/kernel/kernel.go:23-24).
"""
import numpy as _np

from gogp_amd import kernel

#: NaNs with a payload: the sentinels of the kernel tests (tests/test_tile_kernels.py, tests/test_substitution_kernels.py)
#: for every element a launch must neither read nor write -- they come back bit for bit or the test fails
NAN64 = _np.array([0x7FF8DEAD0000BEEF], dtype=_np.uint64).view(_np.float64)[0]
NAN32 = _np.array([0x7FC0BEEF], dtype=_np.uint32).view(_np.float32)[0]

CASES = [
    ("normal1d", 1, kernel.Normal, kernel.ConstantNoise(0.1), [0.3], []),
    ("scaled_rbf", 4, kernel.Scaled(kernel.Normal), kernel.UniformNoise, [1.0, 0.8], [0.1]),
    ("ard_rbf", 5, kernel.Scaled(kernel.ARD(kernel.Normal, 5)), kernel.UniformNoise,
     [1.2, 0.9, 1.0, 1.1, 1.2, 1.3], [0.2]),
    ("matern32", 2, kernel.Scaled(kernel.Matern32), kernel.ScaledNoise(0.01), [1.0, 0.7], [1.5]),
    ("matern52_ref", 3, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, [0.9, 1.1], [0.15]),
    ("matern52_textbook", 3, kernel.Scaled(kernel.Matern52Textbook), kernel.UniformNoise,
     [0.9, 1.1], [0.15]),
    ("periodic", 1, kernel.Scaled(kernel.Periodic), kernel.UniformNoise, [1.0, 0.8, 0.45], [0.2]),
    ("hyperpriors", 1,
     kernel.Sum([kernel.Scaled(kernel.Matern52), kernel.Scaled(kernel.PeriodScaled(kernel.Periodic, 10.0))],
                order=[0, 2, 1, 3, 4]), kernel.ScaledNoise(0.01), [1.0, 0.5, 0.6, 1.3, 0.05], [2.0]),
    ("default_noise", 2, kernel.Scaled(kernel.Matern32), None, [1.0, 0.3], []),
]

#: tutorial/anynoise/kernel/kernel.go:12-35: c*Matern52 with a constant 1e-5 noise that still
#: owns one parameter (used by the priors only).  Kept out of CASES: the committed
#: oracle_vectors.json enumerates CASES.
ANYNOISE = ("anynoise", 1, kernel.Scaled(kernel.Matern52), kernel.ConstantNoiseParam(1e-5 ** 0.5),
            [1.1, 0.6], [0.3])


# ---------------------------------------------------------------------------------------------------------------------
# The schedules the defaults select by size (gogp_amd/csrc/api.hip: superpanel_width, chain_prio_of, chain_split_of,
# GRAPH_EXPLICIT_MAX_NPAD, factorize_t's kinv_fused), at ragged N: tests/test_schedule_regimes_gpu.py and
# tests/golden/make_schedule_regimes.py.  One size on each side of every switch, none a multiple of 256.
# ---------------------------------------------------------------------------------------------------------------------
#: N -> (npad, 256-panels)
REGIME_SIZES = {4400: (4608, 18), 6200: (6400, 25), 8100: (8192, 32), 8300: (8448, 33), 10200: (10240, 40),
                10300: (10496, 41), 12345: (12544, 49)}

#: the thresholds as api.hip states them (a retune there must move a size here, not empty a regime)
REGIME_THRESHOLDS = {"superpanel_head": 4096, "chain_prio": 6144, "chain_split": 8192, "graph_explicit": 8192,
                     "kinv_fused": 10240}


def _ard_theta(D):
    import numpy as np
    return [1.1] + list(np.sqrt(D / 6.0) * (1 + np.arange(D) / (2.0 * D)))


_HYPERPRIORS = [c for c in CASES if c[0] == "hyperpriors"][0]

#: family -> (NDim, Simil, Noise, theta_simil, theta_noise, sizes)
REGIME_FAMILIES = {
    # the suite's standard problem (test_gpu_parity._data, theta = (1.1, 0.6, 0.1))
    "matern52": (3, kernel.Scaled(kernel.Matern52), kernel.UniformNoise, [1.1, 0.6], [0.1], sorted(REGIME_SIZES)),
    # one radial ARD term: the matrix-core reduction of grad_mfma.hip
    "ard_rbf9": (9, kernel.Scaled(kernel.ARD(kernel.Normal, 9)), kernel.UniformNoise, _ard_theta(9), [0.2],
                 [8300, 10300]),
    "hyperpriors": _HYPERPRIORS[1:6] + ([4400],),
}

#: (family, N) of every fp64 case, in the order of the committed record
REGIME_CASES = [(f, n) for f in REGIME_FAMILIES for n in REGIME_FAMILIES[f][5]]

REGIME_M = 300  # test points per case; Produce is asked for the first 1, 64, 65 and all 300 of them


def regime_inputs(family, n):
    """Inputs of one case: the suite's standard data (test_gpu_parity._data) from a seed of its own per (family, N),
    REGIME_M test points, log theta."""
    import numpy as np
    D, _, _, ts, tn, _ = REGIME_FAMILIES[family]
    rng = np.random.default_rng(31000 + 7 * list(REGIME_FAMILIES).index(family) + n)
    X = rng.uniform(0, 1, (n, D))
    y = np.sin(2 * np.pi * X).sum(1) / np.sqrt(D) + 0.1 * rng.normal(size=n)
    y = (y - y.mean()) / y.std()
    Z = rng.uniform(-0.1, 1.1, (REGIME_M, D))
    return X, y, Z, np.log(np.array(list(ts) + list(tn)))


def factor_residual_ratio(L, K):
    """rho = max_ij |L L^T - K|_ij / (gamma_{n+1} (|L| |L|^T)_ij), gamma_k = k u / (1 - k u), u = 2^-53: Higham's
    componentwise bound on a computed Cholesky factor holds with rho <= 1 (Accuracy and Stability of Numerical
    Algorithms, 2nd ed., theorem 10.3).  Returns (rho, (i, j) of the largest ratio).  Two N^3 products in float64 BLAS."""
    import numpy as np
    n = len(K)
    u = 2.0 ** -53
    gamma = (n + 1) * u / (1.0 - (n + 1) * u)
    R = L @ L.T
    R -= K
    np.abs(R, out=R)
    Labs = np.abs(L)
    B = Labs @ Labs.T
    del Labs
    np.divide(R, B, out=R, where=B > 0)  # B_ij = 0 needs (L L^T)_ij = K_ij = 0 exactly: a residual there stays as it is
    del B
    ij = np.unravel_index(int(np.argmax(R)), R.shape)
    return float(R[ij]) / gamma, (int(ij[0]), int(ij[1]))


def tile_instance(prec, mode, mt, nt, k=1, small_below=384):
    """(tile, waves) the tile kernel's launcher picks (gogp_amd/csrc/gemm_plan.h) -- the model that
    tests/test_tile_kernels.py builds its references on and tests/test_gemm_plan_cpu.py pins the plan against."""
    tiles = (mt * (mt + 1) // 2 if mode in ("LOWER", "LAUUM") else mt * nt) * k
    if mode == "LAUUM":
        return 128, 8
    if tiles < small_below or (prec == 64 and 512 < tiles <= 768):
        return 64, 4
    return (128, 8) if tiles >= 3072 else (128, 4)
