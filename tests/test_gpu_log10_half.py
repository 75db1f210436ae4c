"""GPU (-m gpu): c6_log10_half (jaero_amd/csrc/jaero_device.h), the estimate kernels' 0.5 * log10 from halved constants, gives the bits of
0.5 * jd_log10(x) on every family tests/test_gpu_device_math.py measures jd_log10 on.  Both run in one kernel of libjaero_prims.so, with the
product's flags.  The launcher is jc_log10_half and not a jp_ name: the jp_ launchers are the table of tests/device_prims.py, each of which
tests/test_gpu_device_math.py runs, and this one is run here."""
import ctypes as C

import numpy as np
import pytest

import device_prims as DP
from test_gpu_device_math import log10_families

pytestmark = pytest.mark.gpu


def test_half_log10_is_half_of_log10_bit_for_bit():
    L = C.CDLL(DP.PRIMS_LIB)
    L.jc_log10_half.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.jc_log10_half.restype = C.c_int
    fams = log10_families(np.random.default_rng(11))
    assert set(fams) >= {"log-spaced in [1, 1e24]", "1 + k eps, k < 4096", "powers of two", "powers of ten", "around m = sqrt(1/2)"}
    for name, x in fams.items():
        half, prod = np.full(len(x), np.nan), np.full(len(x), np.nan)
        rc = L.jc_log10_half(x.ctypes.data, half.ctypes.data, prod.ctypes.data, len(x))
        assert rc == 0, f"jc_log10_half: hipError {rc}"
        assert np.all(np.isfinite(prod)) and np.all(prod >= 0.0) and prod.max() > 0.0, name
        diff = np.flatnonzero(half.view(np.int64) != prod.view(np.int64))
        assert len(diff) == 0, (name, len(diff), x[diff[:4]], half[diff[:4]], prod[diff[:4]])
