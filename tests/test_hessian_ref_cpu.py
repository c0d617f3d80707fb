"""CPU side of tests/test_hessian_kernels.py and of the analytic tests of tests/test_hessian_gpu.py.
- The closed-form reference (hessian_ref.analytic: per parameter, no slots) agrees with the Richardson-extrapolated
  differences of the analytic gradient within that reference's own tolerance, for every case of the descriptor space.
- The float64 restatements stay below 1e-10 of the long-double ones, relative to the quantity's largest magnitude: the
  condition on the inputs that the GPU tests' allowances rest on.
- The hooks of hessian.hip refuse what a launch cannot honour with GOGP_EARG before the device is touched.
- The manifest: every __global__ of hessian.hip is mapped to the hook that drives it, and that hook is called in the GPU
  kernel test file.  No kernel is exempt."""
import os
import re

import numpy as np
import pytest

import hessian_ref as R
from gogp_amd import _lib, hessian
from gogp_amd import gp as gpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, F64 = np.longdouble, np.float64


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_analytic_agrees_with_the_differences(name):
    H, tol = R.hessian(name, 37)
    A, _ = R.analytic(name, 37)
    ratio = np.abs(A.astype(F64) - H) / tol
    print("%s: largest |analytic - Richardson| / tol = %.3e" % (name, ratio.max()))
    assert np.isfinite(A.astype(F64)).all() and ratio.max() <= 1.0
    assert np.array_equal(A, A.T)


def test_entries_that_vanish_identically():
    # a ConstantNoiseParam's row and column
    for name in ("sum", "hyperpriors"):
        assert R.ALL_CASES[name][2].kind == 2
        A, mag = R.analytic(name, 37)
        assert not A[-1].any() and not A[:, -1].any() and not mag[-1].any()


@pytest.mark.parametrize("n", [1, 37, 64, 129])
def test_float64_restatement_of_the_hessian(n):
    for name in R.ALL_CASES:
        A, mag = R.analytic(name, n)
        A64, _ = R.analytic(name, n, mode="f64")
        top = max(float(np.abs(A).max()), float(mag.max()))
        if top == 0:  # one row, no scale, no noise parameter K depends on: every derivative vanishes
            assert not A64.any(), name
            continue
        rel = float(np.abs(A64.astype(LD) - A).max()) / top
        assert rel < 1e-10, (name, n, rel)


@pytest.mark.parametrize("name", ["ard9", "four", "ard-periodic", "duplicates", "variances", "matern52-u-D1"])
def test_float64_restatement_of_the_kernels(name):
    p = R.kernel_inputs(name, 129)
    a = p["alpha"]
    for K, K64 in zip(R.slot_matrices(p), R.slot_matrices(p, "f64")):
        mag = float(np.abs(K * a.astype(LD)).sum(1).max())
        assert float(np.abs((K64 @ a).astype(LD) - K @ a.astype(LD)).max()) < 1e-10 * mag
        assert float(np.abs(K64.astype(LD) - K).max()) < 1e-10 * max(float(np.abs(K).max()), 1e-300)
    for t, f, k in p["groups"]:
        g = [s[1:3] for s in p["slots"][f:f + k]]
        want, mag = R.moments(p, t, g, g)
        w64, _ = R.moments(p, t, g, g, "f64")
        assert float(np.abs(w64.astype(LD) - want).max()) < 1e-10 * mag.max()


def test_shares_of_the_quantities_the_kernel_tests_judge():
    import test_hessian_kernels as T
    for run in T.runs():
        T.check_shares(*run)


def test_slots_and_groups_of_the_table():
    from gogp_amd import kernel
    seen = set()
    for name, (D, simil, noise, theta) in R.ALL_CASES.items():
        desc = kernel.build_desc(D, simil, noise)
        sl, gr = R.slots(desc)
        assert sorted(s[3] for s in sl) == list(range(desc.ntheta_simil)) and len(theta) == desc.ntheta_simil + noise.NTheta()
        seen.add((len(sl), tuple(k for _, _, k in gr)))
        seen.update(("starts", sl[f][1]) for _, f, _ in gr)
        seen.add(("noise", noise.kind, noise.scale != 1.0))
    assert (10, (3, 3, 3, 1)) in seen and (5, (3, 2)) in seen           # S = 10: 65 trace pairs; 3 + 2 at D = 4
    assert ("starts", R.ARD) in seen and ("starts", R.LEN) in seen and ("starts", R.VALUE) in seen
    assert len(R.trace_pairs(10)) == 65
    assert {("noise", 0, False), ("noise", 1, False), ("noise", 2, False), ("noise", 1, True)} <= seen


# ---- refusals before the device ------------------------------------------------------------------------------------------
EARG, OKS = _lib.GOGP_EARG, (_lib.GOGP_OK, _lib.GOGP_EHIP)


@pytest.fixture(scope="module")
def hooks():
    _lib.build()
    return _lib.hooks()


def status(fn, *args, **kw):
    try:
        fn(*args, device=-1, **kw)
    except RuntimeError as e:
        return int(str(e).rsplit(" ", 1)[1])
    return _lib.GOGP_OK


def base(name="ard-periodic", n=5, npad=64):
    p = R.kernel_inputs(name, n)
    z = np.zeros
    return dict(kp=p["kp"].hook(gpm), X=p["X"], a=p["alpha"], K=z(n * n), n=n, npad=npad, D=p["D"])


def test_hooks_accept_the_valid_calls(hooks):
    b = base()
    n, npad, z = b["n"], b["npad"], np.zeros
    assert status(hessian.kmm_check, b["kp"], 0, [0, 2], [0, 1], b["X"], n, npad, b["K"], n, z(2 * npad * npad)) in OKS
    assert status(hessian.pair_check, b["kp"], 0, [0, 2], [0, 0], [2, 3], [1, 0], b["X"], b["a"], n, npad, b["K"], n, z(25),
                  z(25)) in OKS
    assert status(hessian.kvec_check, b["kp"], 0, [2, 3], [1, 0], b["X"], b["a"], n, npad, z(2 * npad), npad) in OKS
    assert status(hessian.matvec_check, z(npad * npad), b["a"], n, npad, 1, z(npad)) in OKS
    assert status(hessian.dots_check, z(2 * n), z(2 * n), b["a"], n, n, 2, z(6)) in OKS
    assert status(hessian.traces_check, z(2 * npad * npad), 2, b["K"], n, n, npad, [(0, 1), (-1, 1)], z(2), z(2)) in OKS
    assert status(hessian.quad_check, b["K"], n, b["a"], n, npad, z(4), z(4)) in OKS


def test_hooks_refuse(hooks):
    b = base()
    kp, X, a, K, n, npad, z = b["kp"], b["X"], b["a"], b["K"], b["n"], b["npad"], np.zeros
    rad = base("matern32-s-D2")
    bad = [
        # short arrays: X, alpha, Kinv, the outputs
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X[:-1], a, n, npad, K, n, z(25), z(25))),
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a[:-1], n, npad, K, n, z(25), z(25))),
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a, n, npad, K[:-1], n, z(25), z(25))),
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a, n, npad, K, n, z(24), z(25))),
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a, n, npad, K, n, z(25), z(24))),
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a, n, 128, K, n, z(3 * 25 - 1), z(25))),
        (hessian.kvec_check, (kp, 0, [2, 3], [1, 0], X, a, n, npad, z(2 * npad - 1), npad)),
        (hessian.kvec_check, (kp, 0, [2, 3], [1, 0], X, a, n, npad, z(2 * npad), npad - 1)),
        (hessian.kvec_check, (kp, 0, [2], [1], X[:-1], a, n, npad, z(npad), npad)),
        (hessian.kmm_check, (kp, 0, [0], [0], X, n, npad, K, n, z(npad * npad - 1))),
        (hessian.matvec_check, (z(npad * npad - 1), a, n, npad, 1, z(npad))),
        (hessian.matvec_check, (z(npad * npad), a[:-1], n, npad, 1, z(npad))),
        (hessian.matvec_check, (z(npad * npad), a, n, npad, 1, z(npad - 1))),
        (hessian.dots_check, (z(2 * n - 1), z(2 * n), a, n, n, 2, z(6))),
        (hessian.dots_check, (z(2 * n), z(2 * n - 1), a, n, n, 2, z(6))),
        (hessian.dots_check, (z(2 * n), z(2 * n), a, n, n, 2, z(5))),
        (hessian.dots_check, (z(2 * n), z(2 * n), a, n - 1, n, 2, z(6))),
        (hessian.traces_check, (z(2 * npad * npad - 1), 2, K, n, n, npad, [(0, 1)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K[:-1], n, n, npad, [(0, 1)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(0, 1), (1, 1)], z(1), z(2))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(0, 1), (1, 1)], z(2), z(1))),
        (hessian.quad_check, (K[:-1], n, a, n, npad, z(4), z(4))),
        (hessian.quad_check, (K, n, a, n, npad, z(3), z(4))),
        (hessian.quad_check, (K, n, a, n, npad, z(4), z(3))),
        # npad not a multiple of 64, n outside 1 .. npad
        (hessian.pair_check, (kp, 0, [0], [0], [2], [1], X, a, n, 96, K, n, z(75), z(25))),
        (hessian.kvec_check, (kp, 0, [2], [1], X, a, n, 63, z(64), 64)),
        (hessian.matvec_check, (z(100 * 100), a, n, 100, 1, z(100))),
        (hessian.traces_check, (z(2 * 96 * 96), 2, K, n, n, 96, [(0, 1)], z(4), z(1))),
        (hessian.quad_check, (K, n, a, n, 32, z(4), z(4))),
        (hessian.quad_check, (K, n, a, 0, npad, z(4), z(4))),
        (hessian.matvec_check, (z(npad * npad), z(65), 65, npad, 1, z(npad))),
        # nslot out of hess_group_max: 0, 3 on a periodic term, 4 on a radial one
        (hessian.kvec_check, (kp, 0, [], [], X, a, n, npad, z(npad), npad)),
        (hessian.kvec_check, (kp, 0, [0, 2, 2], [0, 0, 1], X, a, n, npad, z(3 * npad), npad)),
        (hessian.pair_check, (kp, 0, [0, 2, 2], [0, 0, 1], [3], [0], X, a, n, npad, K, n, z(25), z(25))),
        (hessian.pair_check, (kp, 0, [3], [0], [0, 2, 2], [0, 0, 1], X, a, n, npad, K, n, z(25), z(25))),
        (hessian.kvec_check, (rad["kp"], 0, [0, 1, 1, 1], [0] * 4, rad["X"], rad["a"], n, npad, z(4 * npad), npad)),
        (hessian.kmm_check, (kp, 0, [0, 2, 2], [0, 0, 1], X, n, npad, K, n, z(3 * npad * npad))),
        # a periodic slot type on a radial term; an unknown type; a dimension or a term out of range
        (hessian.kvec_check, (rad["kp"], 0, [0, 3], [0, 0], rad["X"], rad["a"], n, npad, z(2 * npad), npad)),
        (hessian.pair_check, (rad["kp"], 0, [0], [0], [3], [0], rad["X"], rad["a"], n, npad, K, n, z(25), z(25))),
        (hessian.kmm_check, (rad["kp"], 0, [3], [0], rad["X"], n, npad, K, n, z(npad * npad))),
        (hessian.kvec_check, (kp, 0, [4], [0], X, a, n, npad, z(npad), npad)),
        (hessian.kvec_check, (kp, 0, [2], [2], X, a, n, npad, z(npad), npad)),
        (hessian.kvec_check, (kp, 1, [2], [0], X, a, n, npad, z(npad), npad)),
        # a pair index >= S, below -1, or a second index of -1; no pairs; S out of range
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(0, 2)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(2, 0)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(-2, 0)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [(0, -1)], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 2, K, n, n, npad, [], z(1), z(1))),
        (hessian.traces_check, (z(2 * npad * npad), 0, K, n, n, npad, [(0, 0)], z(1), z(1))),
        (hessian.matvec_check, (z(npad * npad), a, n, npad, 0, z(npad))),
        (hessian.dots_check, (z(2 * n), z(2 * n), a, n, n, 0, z(6))),
    ]
    for i, (fn, args) in enumerate(bad):
        assert status(fn, *args) == EARG, (i, fn.__name__)


# ---- the manifest ------------------------------------------------------------------------------------------------------------
#: kernel -> the hook (gogp_test_hess_<name>, hessian.<name>_check) that drives it through its product launcher
KERNEL_HOOKS = {
    "hess_kmm_kernel": "kmm", "hess_pair_kernel": "pair", "hess_kvec_kernel": "kvec", "hess_matvec_kernel": "matvec",
    "hess_dots_kernel": "dots", "hess_trdot_kernel": "traces", "hess_quad_kernel": "quad",
    "hess_sum_kernel": "traces",  # no launcher of its own: behind pair, quad and traces; 289 partials in test_traces
}
HOOK_TEST = "test_hessian_kernels.py"


def test_every_kernel_of_hessian_hip_is_tested_in_isolation():
    src = open(os.path.join(ROOT, "gogp_amd", "csrc", "hessian.hip")).read()
    src = re.sub(r"//[^\n]*", "", src)
    scan = r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\("
    found = re.findall(scan, src)
    assert len(found) == len(set(found)) == 8
    assert set(found) == set(KERNEL_HOOKS), "a kernel without a hook, or a kernel that is gone: %s" % (set(found) ^ set(KERNEL_HOOKS))
    declared = {name for name, _, _ in _lib.HOOK_SYMBOLS}
    header = open(os.path.join(ROOT, "include", "gogp_testhooks.h")).read()
    common = open(os.path.join(ROOT, "gogp_amd", "csrc", "common.h")).read()
    test = open(os.path.join(ROOT, "tests", HOOK_TEST)).read()
    for k, hook in KERNEL_HOOKS.items():
        assert "gogp_test_hess_" + hook in declared and re.search(r"\bint gogp_test_hess_%s\(" % hook, header), k
        assert re.search(r"\bvoid launch_hess_%s\(" % hook, common), k
        assert "hessian.%s_check(" % hook in test, "no test calls the hook of %s" % k
    # gogp_lml_hessian launches through the launchers alone
    body = src[src.index('extern "C" int gogp_lml_hessian'):]
    assert "GOGP_KLAUNCH" not in body and "hipLaunchKernelGGL" not in body
    probe = "template <int G>\n__global__ __launch_bounds__(256, 2) void new_kernel(int *p) {}\n__global__ void other_kernel() {}"
    assert re.findall(scan, probe) == ["new_kernel", "other_kernel"]
