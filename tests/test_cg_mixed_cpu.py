"""What of "cg_precision" = 32 (cg_mixed.hip, gogp_cg_last_rounds, the hook gogp_test_kmm32) can be checked without a GPU:
the bindings, the entry point's refusal of NULLs, and the hook's refusals before it touches a device.  (A handle needs a
device: the option's own refusals are in tests/test_cg_mixed_gpu.py.)"""
import ctypes

import numpy as np

import gram_ref as R
from gogp_amd import _lib


def test_symbols_exported_and_bound():
    _lib.build()
    assert len(dict((n, a) for n, _, a in _lib.SYMBOLS)["gogp_cg_last_rounds"]) == 5
    assert len(dict((n, a) for n, _, a in _lib.HOOK_SYMBOLS)["gogp_test_kmm32"]) == 23
    assert _lib.lib().gogp_cg_last_rounds is not None and _lib.hooks().gogp_test_kmm32 is not None
    from gogp_amd import gp
    assert callable(gp.kmm32_check)


def test_null_arguments_are_refused():
    _lib.build()
    L = _lib.lib()
    v = [ctypes.c_int32() for _ in range(4)]
    assert L.gogp_cg_last_rounds(None, *[ctypes.byref(q) for q in v]) == _lib.GOGP_EARG
    assert L.gogp_set_option(None, b"cg_precision", 32) == _lib.GOGP_EARG


def test_the_hook_refuses_before_the_device():
    _lib.build()
    from gogp_amd import gp
    kp = R.exact_kp("radial1", 3).hook(gp)
    A, V, part, out = np.zeros(30), np.zeros(10), np.zeros(64), np.zeros(10)

    def call(centre, rows=10, T=1):
        try:
            gp.kmm32_check(kp, A, rows, None, rows, centre, V, 10, T, None, 1, part, out, 10)
        except gp.GogpError as e:
            return e.code
        return None

    assert call(np.zeros(2)) == _lib.GOGP_EARG                     # fewer centres than dimensions
    assert call(np.array([0.0, np.nan, 0.0])) == _lib.GOGP_EARG    # a centre that is not finite
    assert call(np.zeros(3), rows=11) == _lib.GOGP_EARG            # the arrays are held to the sizes
    assert call(np.zeros(3), T=65) == _lib.GOGP_EARG
