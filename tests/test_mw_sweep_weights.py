"""The weight of the shared trunk coordinates in a block sweep of the limb-per-wave sub-step (csrc/core/engine_mw.hpp sweep_weights): the number of
active blocks is a sum of four flags that are exactly 0.f or 1.f, so om = (nact > 1.5) ? (nact + 1) / 2 : 1 takes four values and 1 / om is selected
from four constants instead of divided.  A correctly rounded division (the host's, and the device's IEEE sequence) gives the very same bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sweep_weights") / "libsweep_weights.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "hostbuild", "sweep_weights_host.cpp"), "-o", out])
    L = C.CDLL(out)
    L.hs_sweep_weights.argtypes = [C.c_float, C.POINTER(C.c_float)]
    L.hs_sweep_weights.restype = None
    return L


@pytest.mark.parametrize("nact", [0, 1, 2, 3, 4])
def test_selected_sweep_weights_equal_the_divided_ones(lib, nact):
    out = (C.c_float * 4)()
    lib.hs_sweep_weights(float(nact), out)
    got = np.array(list(out), np.float32)
    om = np.float32(0.5) * (np.float32(nact) + np.float32(1)) if nact > 1.5 else np.float32(1)
    want = np.array([om, np.float32(1) / om], np.float32)          # numpy's float32 division is correctly rounded as well
    print(nact, [hex(int(b)) for b in got.view(np.uint32)], [hex(int(b)) for b in want.view(np.uint32)])
    assert np.array_equal(got[:2].view(np.uint32), got[2:].view(np.uint32))
    assert np.array_equal(got[:2].view(np.uint32), want.view(np.uint32))
    assert om in (np.float32(1), np.float32(1.5), np.float32(2), np.float32(2.5))
